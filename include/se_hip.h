/*
 * se_hip.h -- C ABI of the MI355X (gfx950) dense-fusion hot path.
 *
 * This is the drop-in boundary for supereight's per-frame path
 *     depth image -> voxel-block allocation -> TSDF / occupancy integration -> raycast
 * i.e. what se_denseslam's DenseSLAMSystem::integration() / ::raycasting()
 * (se_denseslam/src/DenseSLAMSystem.cpp:191-268) do on the host.  The reference has no FFI of
 * its own (one process, header-only C++); each entry point below cites the reference
 * interface it replaces.  POD arguments only: the same shared library serves the C++
 * `DenseSLAMSystem` mirror (include/se/DenseSLAMSystem.h, header-only), the ctypes binding
 * (supereight_amd/pipeline.py) and any other FFI.
 *
 * Conventions
 *   - every function returns an int status: >= 0 success (stage functions return 1 = "ran this
 *     frame", 0 = "gated off", like the reference's bool), < 0 = SE_HIP_E_* ; nothing throws,
 *     nothing calls exit(); se_hip_last_error() gives a message for the calling thread.
 *   - 4x4 matrices are 16 floats in COLUMN-MAJOR order, i.e. Eigen::Matrix4f::data().
 *   - k = (fx, fy, cx, cy) as Eigen::Vector4f k in the reference API.  A pose or k holding a NaN or an infinity (or fx, fy = 0) is refused with
 *     SE_HIP_E_INVALID by every stage call: the reference would fuse garbage; this library's parity argument is made for finite rays.
 *   - one handle <-> one caller thread at a time (the reference is not re-entrant either).
 *   - all work is enqueued on one HIP stream per handle; calls that return data to the host
 *     synchronise that stream, the others are asynchronous -- with one exception (the "host gate", dense unsharded
 *     handles): se_hip_alloc_scan / se_hip_integrate / se_hip_frame wait on the HOST until the
 *     raycast behind the previous integration sweep has started on the device (normally less than a frame period; after
 *     20 ms of wall clock the wait turns into hipStreamSynchronize of the handle's stream); a depth upload waits the same way for the raycast
 *     behind the sweep of three uploads ago (the slot it overwrites).  A caller that hands in its own
 *     stream (se_hip_set_stream) must therefore not hold that stream behind work it has not enqueued yet.  SE_HIP_HOST_GATE=0
 *     in the environment selects the event-ordered form, in which no stage call waits on the host.
 *   - SE_HIP_E_CAPACITY is sticky: once a pool, key list or brick segment has overflowed, every later stage call and
 *     se_hip_sync return it (the map / the replicas are no longer what the reference would hold) until se_hip_load_map
 *     re-initialises the map or the caller acknowledges it with se_hip_clear_overflow().
 */
#ifndef SE_HIP_H
#define SE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SE_FIELD_TYPE of the reference (se_denseslam/include/se/volume_traits.hpp:41-72;
 * se_denseslam/CMakeLists.txt:31-50 builds one library per field type) */
#define SE_HIP_FIELD_SDF 0
#define SE_HIP_FIELD_OFUSION 1

#define SE_HIP_OK 0
#define SE_HIP_E_INVALID (-1)   /* bad argument */
#define SE_HIP_E_DEVICE (-2)    /* HIP runtime error */
#define SE_HIP_E_CAPACITY (-3)  /* block / node / key-list pool exhausted */
#define SE_HIP_E_NOGPU (-4)     /* no usable gfx950 device */

typedef struct se_hip_pipeline se_hip_pipeline;

/* Replaces the state set up by DenseSLAMSystem's constructor
 * (se_denseslam/src/DenseSLAMSystem.cpp:65-126: computation_size_, volume_resolution_,
 * volume_dimension_, discrete_vol_ptr_->init(res, dim)). */
typedef struct se_hip_config {
  int32_t width;             /* computation_size_.x() */
  int32_t height;            /* computation_size_.y() */
  int32_t volume_resolution; /* voxels per side; power of two in [64, 4096] */
  float volume_dimension;    /* metres per side */
  int32_t field_type;        /* SE_HIP_FIELD_* */
  int32_t device;            /* HIP device ordinal */
  int64_t max_blocks;        /* capacity of the voxel-block pool; 0 = default (a dense brick grid while it costs <= 64 GiB and a third of the free device memory, else 24 (N/8)^2 pooled bricks) */
  int32_t row_begin;         /* image rows [row_begin,row_end) this handle alloc-scans and */
  int32_t row_end;           /*   raycasts (multi-GPU tile sharding); 0,0 = the whole image */
} se_hip_config;

int se_hip_create(const se_hip_config* cfg, se_hip_pipeline** out);
/* The multi-device form of the constructor (device_ids[]): one row-sharded replica per listed device,
 * replica i owning the i-th share of the image's 8-row tiles (cfg->device / row_begin / row_end are ignored).  The
 * per-frame key-list exchange between the replicas is the caller's (se_hip_alloc_exchange, or se_hip_new_keys_device +
 * se_hip_alloc_commit); one process per GPU with se_hip_create is the deployment this library is measured in. */
int se_hip_create_replicas(const se_hip_config* cfg, const int32_t* device_ids, int32_t n_devices, se_hip_pipeline** out_handles);
int se_hip_destroy(se_hip_pipeline* p);
const char* se_hip_last_error(void);
/* free function synchroniseDevices() is declared but never defined in the reference
 * (se_denseslam/include/se/DenseSLAMSystem.h:418); this is its body. */
int se_hip_sync(se_hip_pipeline* p);
/* Acknowledges a reported SE_HIP_E_CAPACITY (see the conventions above): synchronises, clears the device-side overflow flag and
 * returns the code that was pending (0 = none, 1 = block / node pool, 2 = key list, 3 = brick segment).  The map keeps whatever
 * it lost; the call only lets a caller that has dealt with that (e.g. by reloading the map) carry on. */
int se_hip_clear_overflow(se_hip_pipeline* p);
/* Use an existing hipStream_t (e.g. PyTorch's current stream) instead of the handle's own. */
int se_hip_set_stream(se_hip_pipeline* p, void* hip_stream);
/* The stream the allocation scan (se_hip_alloc_scan) is launched on when it overlaps the previous
 * frame's raycast.  The multi-GPU driver passes the stream its
 * all-gather of the key lists is ordered on, so that scan + exchange of frame f+1 hide behind the
 * raycast of frame f.  NULL = a stream owned by the handle (the default) -- NOT the legacy default stream: a caller whose collective runs on
 * stream 0 (PyTorch's default stream is handle 0) must create a real stream for it and pass that, or scan and collective are unordered. */
int se_hip_set_scan_stream(se_hip_pipeline* p, void* hip_stream);
/* 1 if the key list of se_hip_alloc_scan is produced on the scan stream (overlap on: the default), 0 if on the main
 * stream like every other stage -- in which case work ordered with the scan (an all-gather of its list) belongs on the main
 * stream.  With overlap on, a handle that is row-sharded, writes its list into a caller buffer (se_hip_set_new_keys_buffer)
 * or has an exchange set (se_hip_set_exchange) ALWAYS scans on the scan stream; only a plain single handle whose main
 * stream is idle at the call (a caller that synchronises every frame) gets the scan straight onto the main stream, and
 * nobody else consumes its list.  se_hip_alloc_exchange / se_hip_alloc_commit follow the stream the last scan ran on. */
int se_hip_scan_overlaps(se_hip_pipeline* p);
/* ---- streaming callers: the one-queue schedule (off by default).
 * The reference's loop is integration(f); raycasting(f); integration(f+1); ... (se_apps/src/benchmark.cpp:148-167).  A caller that streams frames
 * without looking at each frame's vertex_ / normal_ can have raycasting(f) and the allocation scan of integration(f+1) run as ONE launch on the
 * handle's stream: with se_hip_set_streaming(p, 1), se_hip_frame and se_hip_raycast_deferred do not enqueue the raycast of a frame but hold it back
 * until the next se_hip_integrate / se_hip_frame / se_hip_alloc_scan, which launches it together with that frame's scan.  ANY other entry point of
 * this header (se_hip_sync, the image getters, se_hip_raycast, se_hip_track, the render calls, ...; not: the depth uploads, se_hip_filter_depth,
 * se_hip_set_new_keys_buffer, se_hip_enable_timing, se_hip_get_launch_counts) launches an outstanding raycast first, so whatever is read THROUGH the API is what the eager
 * schedule gives.  Reading past the API is what the mode cannot make safe: a caller kernel ordered on the handle's stream behind se_hip_frame(f)
 * would find frame f-1's images.  Therefore
 *   - the mode is opt-in (off: se_hip_frame == se_hip_set_depth_device + se_hip_integrate + se_hip_raycast, all enqueued when it returns);
 *   - se_hip_vertex_normal_device on a streaming handle WITHOUT an image ring switches deferral off for good (sticky): raw pointers and deferral
 *     never coexist;
 *   - with an image ring (below) the contract is explicit: slot (f % slots) holds frame f's images once the NEXT se_hip_frame / se_hip_integrate
 *     call (or any flushing call) has returned and the handle's stream has reached that point;
 *   - a caller that turns out to look at every frame -- the reference's loop with tracking on: se_hip_track(f+1) needs raycasting(f)'s images -- gains
 *     nothing from holding raycasts back (they start later and fuse with no scan).  After two held-back raycasts in a row that some other call had
 *     to launch, with no fused launch in between, the handle launches raycasts eagerly again (r06; se_hip_set_streaming(p, 1) re-arms deferral).
 * Handles whose raycast fits the chip in one round of workgroups (640x480: 2 400 of 2 560) fuse; others (statistics on, sharded sweep, larger
 * images) keep the eager two-queue schedule whatever the flag says.  Row-sharded replicas and handles with a caller key buffer or an exchange fuse
 * too: the scan half of the launch writes the caller's list on the MAIN stream, and se_hip_alloc_exchange / se_hip_alloc_commit follow it there
 * (se_hip_scan_overlaps still answers for the scans that do not ride in a raycast's launch: give such a handle the main stream as its scan
 * stream, se_hip_set_scan_stream, so that both kinds are ordered with the caller's collective -- supereight_amd/multi_gpu.py does).
 * se_hip_set_streaming returns 1 if the handle will fuse, 0 if not (or off); se_hip_frame_is_fused reports the same without changing anything. */
int se_hip_set_streaming(se_hip_pipeline* p, int32_t on);
int se_hip_frame_is_fused(se_hip_pipeline* p);
/* vertex_ / normal_ into a caller-owned device ring instead of the handle's own images: the raycast of frame f -- eager, deferred or fused --
 * writes slot f % slots, a slot = [vertex: width*height*3 floats][normal: width*height*3 floats] (se_hip_image_tile_bytes(p, height) bytes), and
 * that slot IS vertex_ / normal_ for every later consumer (se_hip_track, the render calls, the getters) until the next raycast.  This is how a
 * streaming caller keeps every frame's images (tests/test_gpu_stress_parity.py compares each slot of a fused stream with the oracle).
 * NULL, 0 restores the handle's own images (the current images are copied back; synchronises). */
int se_hip_set_image_ring(se_hip_pipeline* p, float* device_ring, int32_t slots);

/* ---- input: float_depth_ (se::Image<float>, metres, row-major x + y*w), produced by
 * preprocessing() in the reference (DenseSLAMSystem.cpp:128-141).
 * Host images (r06): the call copies the caller's buffer into a ring of three pinned host buffers and returns -- like the reference's synchronous
 * preprocessing(), the caller may reuse its buffer at once -- and enqueues NOTHING: the first kernel of the frame that needs float_depth_ (the allocation
 * scan, one thread per pixel; or a one-kernel conversion in front of se_hip_track / se_hip_render_depth / a row-sharded scan) reads the pinned image over
 * PCIe and writes the device image on its way.  No DMA packet, no second queue, no wait for the previous frame: on a streaming handle the input of frame
 * f+1 crosses PCIe inside the launch that raycasts frame f.  The call waits (on the host) only if all three slots are still in flight, i.e. if the caller
 * is three uploads ahead of the device.
 * The depth domain (this call, se_hip_set_depth_device, se_hip_frame, se_hip_frame_tracked, pinned input): ANY float is accepted, and each value does
 * what the reference's arithmetic does with it (tests/test_gpu_depth_domain.py, bit for bit against the oracle):
 *   - 0 and -0 are holes ("no measurement") everywhere.
 *   - A NaN or -inf pixel is a hole for SDF.  A negative pixel is a hole for both sweeps (`depthSample <= 0`), but both allocation scans test
 *     `== 0` only: its band, mirrored behind the camera, still allocates the blocks it crosses inside the volume, and they stay unwritten.
 *   - Under OFusion a NaN or +inf pixel allocates nothing and MARKS THE VOXELS THAT PROJECT ONTO IT FREE (`!(depthSample <= 0)` passes, H(NaN)
 *     clamps to 0.03).  Advice to callers: send 0, not NaN, for "no return" under OFusion.
 *   - +inf and any depth beyond the far side of the volume carve free space along the pixel (sdf = 1; OFusion: free).
 *   - Denormals are depths like any other (not flushed): a band around the camera itself.
 *   - Finite depths must stay below 1000 m in magnitude: the OFusion scan walks the whole ray from the surface back to the camera, dist / step
 *     trips, and beyond some 2^24 steps the reference's own loop no longer advances.  Nothing refuses or clamps a value (yet).
 *   - The reference is undefined (it casts NaN to a pixel index or to int) for +inf depth under se_hip_track / se_hip_frame_tracked and for NaN
 *     under se_hip_render_depth, and so is this library: the tracker forms the same index and READS OUTSIDE THE REFERENCE IMAGES.  Do not hand
 *     +inf to a tracked frame.  NaN, -inf, negative and -0 pixels under tracking are defined: they have no vertex (`d > 0`). */
int se_hip_upload_depth(se_hip_pipeline* p, const float* host_depth_m);
/* mm2metersKernel (se_denseslam/src/preprocessing.cpp:161-188) applied where the image is first read on the device:
 * uint16 millimetres of size (in_w, in_h), an integer multiple of the computation size ("Invalid ratio." = SE_HIP_E_INVALID). */
int se_hip_upload_depth_mm(se_hip_pipeline* p, const uint16_t* host_depth_mm, int32_t in_w, int32_t in_h);
/* Caller-pinned input (opt-in, r06): with se_hip_set_pinned_input(p, 1) an image handed to the two calls above that lies in page-locked host memory
 * (se_hip_host_alloc below, hipHostMalloc, hipHostRegister) is NOT copied: the frame's first kernel reads it over PCIe where the caller keeps it -- a
 * reader that decodes its frames straight into such a buffer (the reference's loop reads a frame per iteration, se_apps/src/benchmark.cpp:115-133) saves
 * the 16 us copy of a 640x480 image per frame.  The price is the reference's synchronous contract: the buffer must stay unmodified until the frame's
 * integration has run on the device -- i.e. until a call that waits for it has returned (se_hip_sync, an image download, se_hip_track of the next
 * frame) or, for a streaming caller, until three further uploads have been accepted (the handle's own ring discipline).  Pageable images are copied as
 * before, whatever the flag says.  se_hip_host_alloc / se_hip_host_free: page-locked host memory without a HIP dependency in the caller (NULL on failure). */
int se_hip_set_pinned_input(se_hip_pipeline* p, int32_t on);
void* se_hip_host_alloc(size_t bytes);
void se_hip_host_free(void* host);
/* Zero-copy: integrate from a depth image already resident in HBM (width*height floats).  The buffer is read by the
 * allocation scan and by the integration sweep of the frame: it must stay untouched until that sweep has finished
 * (se_hip_sync, or work ordered behind se_hip_integrate on the handle's stream).  It must also be COMPLETE when the handle's streams get to
 * it: a producer kernel on another stream is not ordered with them -- hand the handle the producer's stream (se_hip_set_stream) or wait for it. */
int se_hip_set_depth_device(se_hip_pipeline* p, const float* device_depth_m);

/* ---- bool DenseSLAMSystem::integration(const Vector4f& k, unsigned integration_rate, float mu,
 *      unsigned frame)  (DenseSLAMSystem.h:193, DenseSLAMSystem.cpp:206-268); `pose` is the
 *      member pose_ (camera -> world). */
int se_hip_integrate(se_hip_pipeline* p, const float pose[16], const float k[4], uint32_t integration_rate, float mu,
                     uint32_t frame);
/* The same stage split for multi-GPU runs, so that the caller can put the RCCL allgather of the
 * per-rank new-block key lists between the allocation scan and the sweep:
 *   se_hip_alloc_scan     = buildAllocationList / buildOctantList + Octree::allocate for the keys
 *                           found in this handle's image rows (kfusion/alloc_impl.hpp:54-118,
 *                           bfusion/alloc_impl.hpp:56-129, se_core/include/se/octree.hpp:792-856)
 *   se_hip_new_keys_device= the list this scan produced: uint64[0] = count, uint64[1..count] =
 *                           keys in the reference's key format (octant_ops.hpp:49-53)
 *   se_hip_alloc_commit   = Octree::allocate for `nlists` such lists gathered from other ranks
 *                           (device memory, list i at device_lists + i*stride_words)
 *   se_hip_integrate_sweep= projective_map (se_core/include/se/functors/projective_functor.hpp:139-176) */
int se_hip_alloc_scan(se_hip_pipeline* p, const float pose[16], const float k[4], uint32_t integration_rate, float mu,
                      uint32_t frame);
int se_hip_new_keys_device(se_hip_pipeline* p, uint64_t** device_list, int64_t* capacity_words);
/* Make the scan write its list into caller-owned device memory (e.g. the send buffer of the RCCL
 * allgather); capacity_words includes the count word.  NULL restores the internal buffer. */
int se_hip_set_new_keys_buffer(se_hip_pipeline* p, uint64_t* device_list, int64_t capacity_words);
/* The lists must have been produced by work ordered on the stream the allocation scan runs on: the scan stream
 * (se_hip_set_scan_stream) when se_hip_scan_overlaps() is 1 -- the commit kernel is launched there, behind the scan and
 * the caller's all-gather, beside the previous frame's raycast -- and the main stream otherwise.  A new-key list that
 * overflowed (more keys than its capacity) makes the next stage call fail with SE_HIP_E_CAPACITY: the replicas would
 * diverge otherwise. */
int se_hip_alloc_commit(se_hip_pipeline* p, const uint64_t* device_lists, int32_t nlists, int64_t stride_words);
/* Multi-GPU exchange without a host framework in the per-frame path: `nccl_comm` is the ncclComm_t of the caller's
 * communicator (RCCL), `nccl_all_gather` the address of ncclAllGather in the RCCL the process has loaded (the library
 * itself does not link RCCL).  se_hip_alloc_exchange all-gathers the first `words` words of the scan's key list
 * (se_hip_set_new_keys_buffer / the internal list) into recv_device (world * words) on the scan stream and then does
 * se_hip_alloc_commit on the gathered lists.  NULL, NULL switches it off. */
int se_hip_set_exchange(se_hip_pipeline* p, void* nccl_comm, void* nccl_all_gather, int32_t world);
int se_hip_alloc_exchange(se_hip_pipeline* p, uint64_t* recv_device, int64_t words);
int se_hip_integrate_sweep(se_hip_pipeline* p, const float pose[16], const float k[4], uint32_t integration_rate,
                           float mu, uint32_t frame);
/* Sharded sweep -- SURVEY 8(e) option 4, the alternative to the replicated sweep of projective_functor::apply
 * (projective_functor.hpp:139-160) above; measured and priced in DESIGN.md section 7, off by default.  Replica `rank` of
 * `world` updates only the blocks it owns (owner = (bx + by + bz) mod world, block units) and packs, for each of them, its
 * position, its new active flag and -- if any voxel was in view -- its 512 voxels into the caller's send segment of
 * se_hip_sweep_shard_bytes(cap_bricks) bytes (16-byte aligned), cap_bricks a multiple of 64: [u64 counts x 64][u32 records x cap][float vx
 * x 512 x cap][float vy x 512 x cap], counter c over the records [c * cap / 64, (c + 1) * cap / 64).  After the caller's all-gather of the segments (rank order), se_hip_apply_bricks writes the other replicas'
 * records into this replica's map on the main stream; se_hip_brick_exchange issues that all-gather itself
 * (se_hip_set_exchange) on the main stream and then applies.  A segment that overflows makes the next stage call fail with
 * SE_HIP_E_CAPACITY.  OFusion's node values stay replicated (every replica updates every node).  world <= 1 switches it off. */
size_t se_hip_sweep_shard_bytes(size_t cap_bricks);
int se_hip_set_sweep_shard(se_hip_pipeline* p, int32_t rank, int32_t world, void* send_device, size_t cap_bricks);
int se_hip_apply_bricks(se_hip_pipeline* p, const void* recv_device, int32_t world);
int se_hip_brick_exchange(se_hip_pipeline* p, void* recv_device);

/* Full vertex_ / normal_ images on every rank of a row-sharded run: se_hip_raycast of a sharded handle fills
 * only the handle's own image rows, but their consumer -- tracking(), DenseSLAMSystem.cpp:175-177, and the render*() methods --
 * reads the whole images.  A tile = the rows [row_begin, row_end) of a rank, padded to max_rows rows (the largest share of
 * the partition), vertex rows first, then normal rows: se_hip_image_tile_bytes(p, max_rows) bytes.
 *   se_hip_pack_image_tile    copies the handle's own rows of both images into send_device (one tile);
 *   se_hip_apply_image_tiles  writes the other ranks' tiles (recv_device = world tiles in rank order, as an all-gather of the
 *                             packed tiles delivers them; row_begin / row_end = the partition) into this handle's images;
 *   se_hip_gather_images      pack + ncclAllGather on the communicator of se_hip_set_exchange + apply.
 * Everything is enqueued on the main stream, behind the raycast. */
size_t se_hip_image_tile_bytes(se_hip_pipeline* p, int32_t max_rows);
int se_hip_pack_image_tile(se_hip_pipeline* p, void* send_device, int32_t max_rows);
int se_hip_apply_image_tiles(se_hip_pipeline* p, const void* recv_device, int32_t world, int32_t max_rows, const int32_t* row_begin, const int32_t* row_end);
int se_hip_gather_images(se_hip_pipeline* p, void* send_device, void* recv_device, int32_t max_rows, const int32_t* row_begin, const int32_t* row_end);

/* One frame of the loop of se_apps/src/benchmark.cpp:148-167 in one call: hand-over of a device-resident float_depth_
 * (NULL = keep the current depth image), then integration(), then raycasting() with the same pose -- exactly
 * se_hip_set_depth_device + se_hip_integrate + se_hip_raycast (se_hip_raycast_deferred on a streaming handle, see se_hip_set_streaming).
 * Returns bit 0 = integration ran, bit 1 = raycasting ran (or is held back).  The depth image handed over must stay valid until the next
 * call (the scan and the sweep read it asynchronously). */
int se_hip_frame(se_hip_pipeline* p, const float* device_depth_m, const float pose[16], const float k[4], uint32_t integration_rate,
                 float mu, uint32_t frame);

/* ---- bool DenseSLAMSystem::raycasting(const Vector4f& k, float mu, unsigned frame)
 *      (DenseSLAMSystem.h:212, DenseSLAMSystem.cpp:191-204) -> vertex_, normal_ */
int se_hip_raycast(se_hip_pipeline* p, const float pose[16], const float k[4], float mu, uint32_t frame);
/* raycasting() of a streaming caller (se_hip_set_streaming): same gate, same result, but the launch is held back until the next
 * se_hip_integrate / se_hip_frame (one launch with that frame's allocation scan) or any flushing call; on a handle that does not fuse it IS
 * se_hip_raycast.  include/se/DenseSLAMSystem.h's raycasting() calls this one. */
int se_hip_raycast_deferred(se_hip_pipeline* p, const float pose[16], const float k[4], float mu, uint32_t frame);
/* vertex_ / normal_ : se::Image<Eigen::Vector3f>, packed 12 bytes per pixel, world frame */
int se_hip_download_vertex_normal(se_hip_pipeline* p, float* host_vertex_xyz, float* host_normal_xyz);
/* The device images themselves (zero-copy consumers).  They are current when the call returns (an outstanding deferred raycast is launched first)
 * and are rewritten by the next raycast on the handle's stream.  On a streaming handle without an image ring the call ends deferral for good
 * (see se_hip_set_streaming); with a ring it returns the slot of the last raycast. */
int se_hip_vertex_normal_device(se_hip_pipeline* p, float** device_vertex_xyz, float** device_normal_xyz);

/* ---- "next" row f-2: bool DenseSLAMSystem::tracking(const Vector4f& k, float icp_threshold,
 *      unsigned tracking_rate, unsigned frame)  (DenseSLAMSystem.h:173, DenseSLAMSystem.cpp:143-189):
 *      half-sample pyramid of the current depth image, depth2vertex / vertex2normal per level, ICP against vertex_ /
 *      normal_ of the last se_hip_raycast, checkPoseKernel.  The ICP loop is device-resident: one launch per iteration
 *      (k_icp_iter: the previous iteration's final sums + updatePoseKernel -- 6x6 Cholesky solve, SE3 exponential, pose update,
 *      convergence test -- as a prologue, then trackKernel + reduceKernel's partial sums) and a last launch that is k_icp_finish (the
 *      last iteration's sums and update, checkPoseKernel, the host record) in its first workgroup and tracking_result_ in the others;
 *      the pyramid is one launch (copy + two half-samplings), vertices + normals of all levels another.  The call waits on the host
 *      once for the result; while it enqueues a level's iterations it stays two launches ahead of the device and stops enqueuing a
 *      level that has converged (the launches left out would have returned at once; SE_HIP_ICP_LOOKAHEAD=0: all up front).
 *      A row-sharded handle must have the peers' rows of vertex_ / normal_ (se_hip_gather_images or se_hip_apply_image_tiles
 *      after the raycast): SE_HIP_E_INVALID otherwise.  se_hip_download_track: `result` of every pixel and error / J of the
 *      accepted ones are the reference's; its rejected pixels keep leftovers of earlier iterations there, zeros here.
 *      pose_inout = pose_ (updated in place; restored if the check fails); pyramid = iterations per
 *      level, finest first (default {10, 5, 4}).  Returns 1 = tracked, 0 = gated off or rejected. */
int se_hip_track(se_hip_pipeline* p, const float k[4], float icp_threshold, uint32_t tracking_rate, uint32_t frame,
                 const int32_t* pyramid, int32_t n_levels, float pose_inout[16]);
/* One frame of the reference's loop with tracking on (se_apps/src/benchmark.cpp:115-150) in one call:
 *   float_depth_ = device_depth_m (NULL: keep);  tracked = tracking();  if (tracked || frame <= 3) integration();  raycasting();
 * pose_inout: pose_ (in), pose_ after tracking (out).  Returns bit 0: integration ran, bit 1: raycasting ran, bit 2: tracked;
 * < 0 on error.  Same results as se_hip_set_depth_device + se_hip_track + se_hip_integrate + se_hip_raycast. */
int se_hip_frame_tracked(se_hip_pipeline* p, const float* device_depth_m, const float k[4], float icp_threshold, uint32_t tracking_rate,
                         const int32_t* pyramid, int32_t n_levels, float pose_inout[16], uint32_t integration_rate, float mu, uint32_t frame);
/* preprocessing(..., filterInput) (DenseSLAMSystem.cpp:128-141): when on, se_hip_track works on
 * bilateralFilterKernel(float_depth_) (preprocessing.cpp:41-89, gaussian_ of DenseSLAMSystem.cpp:111-118)
 * instead of float_depth_ itself; integration always uses the unfiltered image, as in the reference.
 * The reference's expf (libm-specific in its last bit) is defined as the correctly rounded exponential, in the kernel and in the
 * Gaussian table, so the filtered image is the parity oracle's bit for bit, NaN, infinite, negative and denormal pixels included. */
int se_hip_filter_depth(se_hip_pipeline* p, int32_t on);
/* scaled_depth_[level] as built by the last se_hip_track ((width >> level) x (height >> level) floats). */
int se_hip_download_scaled_depth(se_hip_pipeline* p, int32_t level, float* host_out);
/* tracking_result_ (TrackData {int result; float error; float J[6];} per pixel, commons.h:249-253) and
 * row 0 of reduction_output_ (32 floats) of the last ICP iteration; iterations run in the last call. */
int se_hip_download_track(se_hip_pipeline* p, void* host_trackdata, float host_reduce32[32], int32_t* iterations);

/* ---- "next" row f-3: the render*() methods (DenseSLAMSystem.h:241-286, DenseSLAMSystem.cpp:274-300;
 *      kernels se_denseslam/src/rendering.cpp:111-283).  Output: width*height RGBW bytes (host).
 *      se_hip_render_volume: view_pose = *viewPose_ (re-raycasts with far = 2*farPlane when it is not
 *      approximately raycast_pose_, else shades vertex_/normal_); light = its translation, ambient 0.1;
 *      mu = the constructor's config.mu; returns 1 = rendered, 0 = gated off (frame % rate != 0).
 *      Domain: largestep is the step the SDF march takes at a voxel of weight 0 (t += largestep, kfusion/rendering_impl.hpp:47-52), as in
 *      the reference; it is not checked.  A largestep of 0, or below half an ulp of 2*farPlane (about 5e-7), leaves t where it is: the
 *      march then never ends, in the reference and in this kernel alike.  Pass a largestep that advances t (the reference's: 0.75 * mu). */
int se_hip_render_volume(se_hip_pipeline* p, uint8_t* host_rgbw, const float view_pose[16], const float k[4], float mu, float largestep,
                         uint32_t frame, uint32_t raycast_rendering_rate);
int se_hip_render_depth(se_hip_pipeline* p, uint8_t* host_rgbw);
int se_hip_render_track(se_hip_pipeline* p, uint8_t* host_rgbw);

/* ---- map read-back: what getMap() exposes as a host se::Octree
 *      (DenseSLAMSystem.h:295; se_core/include/se/octree.hpp:898-914 save layout). */
int se_hip_counts(se_hip_pipeline* p, int32_t* n_blocks, int32_t* n_nodes);
/* What the map costs on the device (no reference counterpart: MemoryPool grows on the host heap, se_core/include/se/utils/memory_pool.hpp:64-95):
 * out[0] = 1 dense brick grid / 0 pooled bricks, out[1] = brick slots, out[2] = bytes of the voxel bricks, out[3] = bytes of everything the handle
 * holds on the device (bricks, index pyramid, bitmaps, lists, key buffers, images, input ring).  Does not touch the device. */
int se_hip_memory_info(se_hip_pipeline* p, int64_t out[4]);
/* blocks sorted by key: coords[n][3] (min corner, voxels), x[n][512], y[n][512] (voxel index
 * x + 8y + 64z, se_core/include/se/node.hpp:139-144), active[n] */
int se_hip_download_blocks(se_hip_pipeline* p, int32_t* coords, float* x, float* y, uint8_t* active);
/* internal nodes sorted by key: code[n] (key = code|level), side[n], x[n][8], y[n][8] (value_[8]) */
int se_hip_download_nodes(se_hip_pipeline* p, uint64_t* code, uint32_t* side, float* x, float* y);

/* ---- batched point queries against the resident map: the reference's map read interface VolumeTemplate
 *      (se_denseslam/include/se/continuous/volume_template.hpp:77-102) for N points in metres at once, without getMap().
 * Voxel coordinates of a point p: q = s * p per axis, s = (float)size / dim (a float division; no FMA anywhere), v = (int)q (truncation).
 *   fine[n][2]   (x, y)  VolumeTemplate::get(p) = Octree::get_fine(v): voxel v, or initValue() if its block is not allocated.
 *   coarse[n][2] (x, y)  VolumeTemplate::operator[](p) = Octree::get(v) (octree.hpp:335-355): voxel v if its block exists, else value_[childid]
 *                        of the deepest existing node on the path from the root (OFusion's multi-resolution free space).
 *   interp[n]            VolumeTemplate::interp(p, x) = Octree::interp(q) (octree.hpp:541-563), bit for bit.
 *   grad[n][3]           VolumeTemplate::grad(p, x) = Octree::grad(q) (octree.hpp:652-737), scaled by 0.5 * dim / size as there, bit for bit.
 *   status[n] (uint8)    bit 0: v lies in [0, size)^3; bit 1: the block holding v is allocated; bit 2: all eight voxels interp reads
 *                        (corners max(floor(q), 0) + {0, 1} per axis) lie in allocated blocks -- the interpolated value comes from observed
 *                        blocks only.
 * y is returned as float, as se_hip_download_blocks does: the weight for SDF, the last-update time for OFusion.
 * Defined beyond the reference, whose unchecked tree walk is undefined there:
 *   - v outside [0, size)^3: fine = coarse = initValue(), status bit 0 clear; interp / grad are still Octree::interp / Octree::grad with
 *     missing blocks (outside the volume none exists): empty().x / initValue().x corners as the reference's gather rules say.
 *   - a non-finite point, or |q| >= 2^20 on any axis: status = 0, fine = coarse = initValue(), interp = empty().x, grad = (0, 0, 0); no map
 *     memory is read.
 * A null output pointer means "not wanted"; at least one must be set.  Both entries answer for the map after everything enqueued before them
 * (a scan that ran on the side stream included), refuse n < 0, a null points pointer with n > 0 or no output with SE_HIP_E_INVALID (n == 0 is a
 * no-op), and report a sticky SE_HIP_E_CAPACITY like the other read-back calls.  No launch counter (SE_HIP_K_*) counts them.
 *   se_hip_query_points       device arrays (points [n][3] float, outputs as above); enqueued on the handle's stream, asynchronous like the
 *                             stage calls -- the outputs are complete once the stream has reached that point (se_hip_sync).
 *   se_hip_query_points_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
typedef struct se_hip_query_out {
  float* fine;      /* [n][2] */
  float* coarse;    /* [n][2] */
  float* interp;    /* [n]    */
  float* grad;      /* [n][3] */
  uint8_t* status;  /* [n]    */
} se_hip_query_out;
int se_hip_query_points(se_hip_pipeline* p, const float* device_points_m, int64_t n, const se_hip_query_out* device_out);
int se_hip_query_points_host(se_hip_pipeline* p, const float* host_points_m, int64_t n, const se_hip_query_out* host_out);

/* ---- batched collision queries for axis-aligned boxes against the resident map: the reference's map read algorithm
 *      se::geometry::collides_with (se_core/include/se/geometry/octree_collision.hpp:74-167, overlap test aabb_collision.hpp),
 *      for N boxes at once, without getMap().  The host restatement of that function is include/se/octree_collision.hpp.
 * Box: int32 lo[3], side[3] in voxel units (collides_with(map, bbox = lo, side, test)).  A box with side < 1 on any axis, or with any
 *   coordinate of lo or lo + side outside [-2^30, 2^30], gets status SE_HIP_COLLISION_INVALID and reads no map memory.
 * Voxel classification (the reference passes a functor; here a parameter struct).  v = (x, y), y read as float as se_hip_download_blocks
 *   returns it (the SDF weight byte converted; OFusion's y as stored):
 *     unseen    if x == initValue().x && y == initValue().y (the rule of the reference's own test functor: SDF {1, 0}, OFusion {0, 0});
 *     occupied  else if (occupied_above ? x > threshold : x < threshold);
 *     empty     otherwise.
 * Status codes follow the order of se::geometry::collision_status; combining two statuses takes the smaller code (the reference's
 *   update_status: empty < unseen < occupied by severity).
 * Modes:
 *   SE_HIP_COLLIDE_STRICT     B = [lo, lo + side) per axis (half open).  status = min over the voxels v of B ∩ [0, size)^3 of
 *                             classify(Octree::get(v)) -- the voxel if its block is allocated, else value_[child] of the deepest existing
 *                             node on the path (exactly the coarse output of se_hip_query_points at v).  Any part of B outside the volume
 *                             counts as unseen; a box entirely outside is unseen.
 *   SE_HIP_COLLIDE_REFERENCE  exactly what the reference's collides_with returns, quirks included (deliberate parity):
 *                             - inclusive overlap test on integer midpoints, |(b + be/2) - (a + ae/2)| <= (ae + be)/2, for octants and for
 *                               voxels (edge 1): a box of side 2 touches 3 voxels per axis (evaluated without int32 overflow);
 *                             - an absent overlapping child is judged by its parent's value_[0], not value_[child];
 *                             - a visited leaf's status replaces the running status instead of being merged into it;
 *                             - the root is always visited and is not itself overlap-tested; a node without children adds nothing.
 *                             The traversal is a stack DFS that visits children in order 7..0, so the result has a closed form (DESIGN.md
 *                             4.7): with L* the visited leaf of smallest Morton code, result = min(class(L*), ev(Q) for the visited internal
 *                             nodes Q whose octant ends at or before L*'s code); without a visited leaf, the min of every ev(Q) from empty.
 *                             ev(Q) = classify(Q.value_[0]) if Q has children and an overlapping absent child.  Only L*'s voxels are read.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * boxes or status pointer with n > 0, a null test, a non-finite threshold, occupied_above other than 0 / 1 and an unknown mode with
 * SE_HIP_E_INVALID (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the map, the images and
 * the launch counters (SE_HIP_K_*) alone.
 *   se_hip_collide_boxes       device arrays (boxes [n][6] int32: lo xyz, side xyz; status [n] uint8); enqueued on the handle's stream,
 *                              asynchronous like the stage calls.
 *   se_hip_collide_boxes_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_COLLISION_OCCUPIED 0
#define SE_HIP_COLLISION_UNSEEN 1
#define SE_HIP_COLLISION_EMPTY 2
#define SE_HIP_COLLISION_INVALID 255
#define SE_HIP_COLLIDE_STRICT 0
#define SE_HIP_COLLIDE_REFERENCE 1
typedef struct se_hip_collide_test {
  float threshold;
  int32_t occupied_above;   /* 1: x > threshold is occupied (OFusion log-odds), 0: x < threshold (SDF) */
} se_hip_collide_test;
int se_hip_collide_boxes(se_hip_pipeline* p, const int32_t* device_boxes, int64_t n, const se_hip_collide_test* test, int32_t mode,
                         uint8_t* device_status);
int se_hip_collide_boxes_host(se_hip_pipeline* p, const int32_t* host_boxes, int64_t n, const se_hip_collide_test* test, int32_t mode,
                              uint8_t* host_status);

/* ---- batched collision queries for boxes moved along straight segments: "may this robot move from A to B, and if not, how far?" for N
 *      motions at once, without getMap().  Not in the reference; built on its Octree::get and on the classification above.  The host
 *      restatement and the literal definition are include/se/motion_collision.hpp.
 * Motion: nine int32, lo xyz, side xyz, d xyz, in voxels (motions [n][9]).  The box [lo, lo + side) is translated by t * d for t in [0, 1].
 * Touched: a cube with integer corner c and side s (a voxel: s = 1) is touched iff some t in [0, 1] has, on every axis k,
 *     lo_k + t d_k < c_k + s   and   lo_k + side_k + t d_k > c_k.
 *   The inequalities are open: a face sliding exactly along a voxel face touches nothing; for d = 0 the touched voxels are exactly those of the
 *   half-open box of SE_HIP_COLLIDE_STRICT.  An axis with d_k = 0 gives a static condition, every other axis an open interval with rational ends
 *   over |d_k|; with L the largest lower end and U the smallest upper end the cube is touched iff L < U, L < 1 and U > 0, and its entry
 *   parameter is t_in = max(0, L).  Every comparison is exact (cross-multiplication in 64-bit integers): nothing depends on a step or a rounding.
 * Classification: exactly that of se_hip_collide_boxes in strict mode -- `test` applied to Octree::get(v) (the voxel, or value_[child] of the
 *   deepest existing node); voxels outside [0, size)^3 are unseen.
 * A motion with side < 1 on any axis, or with any coordinate of lo, lo + side, lo + d or lo + side + d outside [-2^20, 2^20], is invalid and
 *   reads no map memory.  (The bound keeps every numerator and denominator of the intervals below 2^24 -- exactly representable as floats --
 *   and every cross product inside int64.)
 * Outputs (se_hip_motion_out; a null t_first means "not wanted", status is required):
 *   status[n]   (uint8) the min over all touched voxels of their class, SE_HIP_COLLISION_*; SE_HIP_COLLISION_INVALID for an invalid motion.
 *   t_first[n]  (float) with stop_at in {SE_HIP_COLLISION_OCCUPIED, SE_HIP_COLLISION_UNSEEN}, a voxel blocks when its class is <= stop_at;
 *               t_first is the smallest t_in over the touched blocking voxels, those outside the volume included, returned as
 *               (float)num / (float)den of the exact rational (both terms are exactly representable, so the quotient depends on the value
 *               only): 0 when the motion is blocked at its start, SE_HIP_MOTION_FREE (2.0f) when nothing blocks, -1.0f for an invalid motion.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * out, a null motions or status pointer with n > 0, a null test, a non-finite threshold, occupied_above other than 0 / 1 and a stop_at other
 * than the two above with SE_HIP_E_INVALID (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the
 * map, the images and the launch counters (SE_HIP_K_*) alone.
 *   se_hip_collide_motions       device arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_collide_motions_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_MOTION_FREE 2.0f
typedef struct se_hip_motion_out {
  uint8_t* status;  /* [n] */
  float* t_first;   /* [n] */
} se_hip_motion_out;
int se_hip_collide_motions(se_hip_pipeline* p, const int32_t* device_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                           const se_hip_motion_out* device_out);
int se_hip_collide_motions_host(se_hip_pipeline* p, const int32_t* host_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                                const se_hip_motion_out* host_out);

/* ---- batched clearance queries: "how far is this box from the nearest obstacle, and where is that obstacle?" for N boxes at once, without
 *      getMap().  Not in the reference; built on its Octree::get and on the classification above.  The host restatement and the literal
 *      definition are include/se/clearance.hpp.
 * Query: seven int32, lo xyz, side xyz, r_max, in voxels (queries [n][7]).  The box is [lo, lo + side) per axis.
 * Distance: for a cube with integer corner c and side s (a voxel: s = 1) the gap on axis k is
 *     g_k = max(0, c_k - (lo_k + side_k), lo_k - (c_k + s))   and   d2 = g_x^2 + g_y^2 + g_z^2,
 *   the squared Euclidean distance between the two closed sets: 0 when they overlap or touch.  Everything is integer arithmetic; nothing
 *   depends on a rounding.
 * Classification: exactly that of se_hip_collide_boxes in strict mode -- `test` applied to Octree::get(v) (the voxel, or value_[child] of the
 *   deepest existing node; a pending entry counts as absent); every voxel of Z^3 outside [0, size)^3 is unseen.  With stop_at in
 *   {SE_HIP_COLLISION_OCCUPIED, SE_HIP_COLLISION_UNSEEN}, a voxel blocks when its class is <= stop_at, as in se_hip_collide_motions.
 * A query with side < 1 on any axis, with r_max outside [0, 32767], or with any coordinate of lo or lo + side outside [-2^19, 2^19], is
 *   invalid and reads no map memory.  (The bounds keep d2 below 2^30 and every witness coordinate below 2^20 in magnitude: the pair
 *   (d2, z, y, x) packs into 32 + 63 bits.)
 * Outputs (se_hip_clearance_out; a null nearest means "not wanted", d2 is required):
 *   d2[n]          (int32) the smallest d2 over all blocking voxels with d2 <= r_max^2, those outside the volume included;
 *                  SE_HIP_CLEARANCE_NONE if there is none, SE_HIP_CLEARANCE_INVALID for an invalid query.
 *   nearest[n][3]  (int32, x y z) among the blocking voxels that attain that d2 (a finite set), the smallest in (z, y, x) lexicographic
 *                  order; (INT32_MIN, INT32_MIN, INT32_MIN) for NONE and for INVALID.
 *   The definition is per voxel: it does not depend on how the tree happens to be subdivided.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * out, a null queries or d2 pointer with n > 0, a null test, a non-finite threshold, occupied_above other than 0 / 1 and a stop_at other
 * than the two above with SE_HIP_E_INVALID (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the
 * map, the images and the launch counters (SE_HIP_K_*) alone.
 *   se_hip_clearance_boxes       device arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_clearance_boxes_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_CLEARANCE_NONE (-1)
#define SE_HIP_CLEARANCE_INVALID (-2)
typedef struct se_hip_clearance_out {
  int32_t* d2;       /* [n]    */
  int32_t* nearest;  /* [n][3] */
} se_hip_clearance_out;
int se_hip_clearance_boxes(se_hip_pipeline* p, const int32_t* device_queries, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                           const se_hip_clearance_out* device_out);
int se_hip_clearance_boxes_host(se_hip_pipeline* p, const int32_t* host_queries, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                                const se_hip_clearance_out* host_out);

/* ---- column projections: "give me the 2D grid" -- the occupancy of a height band per cell (a costmap), the highest occupied voxel per cell
 *      (an elevation map), the lowest one above some height (a ceiling map), the cells whose band still holds unseen voxels (a 2D frontier)
 *      -- in one call, without getMap().  Not in the reference; built on its Octree::get and on the classification above.  The host
 *      restatement and the literal definition are include/se/project_columns.hpp.
 * Request (se_hip_project_request, a host struct that is copied into the launch), in voxels:
 *   axis      0, 1 or 2: the axis w the columns run along.  The two remaining axes, in ascending order, are u (the fastest output index) and
 *             v:  axis 2: u = x, v = y;  axis 1: u = x, v = z;  axis 0: u = y, v = z.
 *   lo, side  the footprint [lo[0], lo[0] + side[0]) on u and [lo[1], lo[1] + side[1]) on v.
 *   n_layers  L, 1 .. SE_HIP_PROJECT_MAX_LAYERS; layers[l] = {a_l, b_l}: the half-open interval [a_l, b_l) along w.  Layers may overlap.
 *   stop_at   SE_HIP_COLLISION_OCCUPIED or SE_HIP_COLLISION_UNSEEN, with the meaning it has in se_hip_collide_motions.
 * Definition, per voxel of Z^3 and independent of how the tree happens to be subdivided: cell (l, j, i) is the set of voxels with
 *   u-coordinate lo[0] + i, v-coordinate lo[1] + j and w in [a_l, b_l).  Classification is exactly that of se_hip_collide_boxes in strict mode
 *   -- `test` applied to Octree::get(v) (the voxel, or value_[child] of the deepest existing node; a pending index entry counts as absent);
 *   every voxel outside [0, size)^3 is unseen.  A voxel blocks when its class is <= stop_at.
 * Outputs (se_hip_project_out), each [L][side[1]][side[0]]; status is required, a null pointer for another array means "not wanted":
 *   status  (uint8) the min class over the cell's voxels, SE_HIP_COLLISION_*: the strict status of the cell's 1 x 1 x (b - a) box.
 *   first   (int32) the smallest w of a blocking voxel of the cell;  last  (int32) the largest;  both SE_HIP_PROJECT_NONE (INT32_MIN) when no
 *           voxel of the cell blocks.  Along z with stop_at occupied, last is the elevation map and first the ceiling.
 *   count   (int32) the number of blocking voxels of the cell.
 *   Blocking voxels outside the volume are included: a cell may stick out of the volume, or lie wholly outside it.  Those parts are
 *   answered in closed form, so a layer [-2^20, 2^20) costs no more than the volume's own height.
 * The whole call is refused with SE_HIP_E_INVALID, and reads no map memory, for: a null request, test, out or status pointer; an axis outside
 * 0 .. 2; a side < 1; a_l >= b_l; any of lo, lo + side, a_l, b_l outside [-2^20, 2^20]; L outside 1 .. 16; L * side[0] * side[1] > 2^28; a
 * stop_at other than the two above; a non-finite threshold; occupied_above other than 0 / 1.  Nothing is written to the outputs then.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), report a sticky
 * SE_HIP_E_CAPACITY like the other read-back calls, and leave the map, the images and the launch counters (SE_HIP_K_*) alone.
 *   se_hip_project_columns       device output arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_project_columns_host  host output arrays; staged through a device buffer the handle keeps (and grows); synchronises before it
 *                                returns. */
#define SE_HIP_PROJECT_NONE INT32_MIN
#define SE_HIP_PROJECT_MAX_LAYERS 16
typedef struct se_hip_project_request {
  int32_t axis;
  int32_t lo[2];        /* u, v */
  int32_t side[2];      /* u, v */
  int32_t n_layers;
  int32_t layers[SE_HIP_PROJECT_MAX_LAYERS][2];
  int32_t stop_at;
} se_hip_project_request;
typedef struct se_hip_project_out {
  uint8_t* status;  /* [L][side[1]][side[0]] */
  int32_t* first;
  int32_t* last;
  int32_t* count;
} se_hip_project_out;
int se_hip_project_columns(se_hip_pipeline* p, const se_hip_project_request* request, const se_hip_collide_test* test,
                           const se_hip_project_out* device_out);
int se_hip_project_columns_host(se_hip_pipeline* p, const se_hip_project_request* request, const se_hip_collide_test* test,
                                const se_hip_project_out* host_out);

/* ---- the distance field of a region: "how far is every position of this region from the nearest obstacle?" -- the ESDF a gradient-based
 *      planner differentiates, or the C-space map of a box robot -- in one call, without getMap().  Not in the reference; it is the answer of
 *      se_hip_clearance_boxes for every voxel of the region, bit for bit.  The host restatement and the literal definition are
 *      include/se/distance_field.hpp.
 * Request (se_hip_field_request, a host struct that is copied into the launch), in voxels:
 *   lo, side  the region [lo, lo + side) per axis (x, y, z).
 *   robot     the side of the box whose min corner is placed at each voxel of the region; (1, 1, 1) gives the plain voxel field.
 *   r_max, stop_at  as in se_hip_clearance_boxes (r_max at most 255 here).
 * Outputs (se_hip_field_out; a null nearest means "not wanted", d2 is required):
 *   d2[side z][side y][side x]          (int32) entry (k, j, i) is exactly the d2 that se_hip_clearance_boxes returns for the query
 *                                       (lo + (i, j, k), robot, r_max) under the same test and stop_at, SE_HIP_CLEARANCE_NONE included.
 *                                       Blocking voxels outside the region count, and so do those outside the volume (unseen): the region
 *                                       may stick out of the volume or lie wholly outside it.
 *   nearest[side z][side y][side x][3]  (int32, x y z) that query's nearest, with the same (z, y, x) tie rule; INT32_MIN three times for NONE.
 *   Classification, the gap formula, "a pending index entry counts as absent" and the independence of how the tree happens to be subdivided
 *   are as in se_hip_clearance_boxes.
 * The whole call is refused with SE_HIP_E_INVALID, and then reads no map memory and writes nothing, for: a null request, test, out or d2
 * pointer; a side or robot entry < 1; a robot entry > 256; r_max outside [0, 255]; any of lo, lo + side + robot outside [-2^19, 2^19] (so
 * that every voxel's query is a valid clearance query); side[0] * side[1] * side[2] > 2^24; side[0] * D1 * D2 > 2^28 with D_k = side[k] +
 * robot[k] + 2 r_max + 1 (the entries of the x pass's work buffer: the call keeps side[0] * D1 * D2 * 2 + side[0] * side[1] * D2 * 4 bytes
 * in the handle's staging buffer, at most 512 MiB + 1 GiB); a stop_at, threshold or occupied_above that se_hip_clearance_boxes refuses.
 * A third work buffer, the blocking bits, is not bounded by a refusal of its own: one bit per voxel of the block-aligned hull of the
 * D0 x D1 x D2 domain, rows along x padded to 8 bytes, i.e. at most ((D0 + 14) / 8 + 8) * (D1 + 14) * (D2 + 14) bytes.  For regions that are
 * not thin along x it is the smallest of the three; for a thin one with a large robot and r_max it is the largest -- side (1, 4096, 4096)
 * with robot 256 and r_max 255 is a valid request that needs 2.3 GB of bits, and under the refusals above the worst case (side[0] = 1, D0 =
 * 768, D1 * D2 = 2^28) stays below 32 GiB.  A staging buffer the device cannot provide fails the call with SE_HIP_E_DEVICE before anything
 * is launched or written.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), report a sticky
 * SE_HIP_E_CAPACITY like the other read-back calls, and leave the map, the images and the launch counters (SE_HIP_K_*) alone.
 *   se_hip_distance_field       device output arrays; enqueued on the handle's stream, asynchronous like the stage calls -- but for one
 *                               thing: when the work buffers need a larger staging buffer than the handle holds, growing it waits for the
 *                               work enqueued before (the old buffer may still be read).
 *   se_hip_distance_field_host  host output arrays; staged through the same buffer; synchronises before it returns. */
typedef struct se_hip_field_request {
  int32_t lo[3];      /* x, y, z */
  int32_t side[3];
  int32_t robot[3];
  int32_t r_max;
  int32_t stop_at;
} se_hip_field_request;
typedef struct se_hip_field_out {
  int32_t* d2;       /* [side z][side y][side x]    */
  int32_t* nearest;  /* [side z][side y][side x][3] */
} se_hip_field_out;
int se_hip_distance_field(se_hip_pipeline* p, const se_hip_field_request* request, const se_hip_collide_test* test,
                          const se_hip_field_out* device_out);
int se_hip_distance_field_host(se_hip_pipeline* p, const se_hip_field_request* request, const se_hip_collide_test* test,
                               const se_hip_field_out* host_out);

/* ---- the reachability field of a region: "can the robot get from here to there at all, how long is the way, and which way does it go?" --
 *      a wavefront / NF1 navigation function over the C-space of the box robot that se_hip_distance_field models, in one call, without
 *      getMap() and a flood fill on the host.  Not in the reference: the definition below is the contract.  Everything is integer.  The
 *      literal definition and a host restatement of the device's tile scheme are include/se/reach_field.hpp.
 * Request (se_hip_reach_request, a host struct), in voxels:
 *   lo, side  the region [lo, lo + side) per axis (x, y, z).
 *   robot     the side of the box whose min corner stands at a position.
 *   stop_at   as in se_hip_distance_field.
 *   n_seeds   1 .. 255.
 *   seeds     a HOST pointer, in both entries, to [n_seeds][3] int32 (x, y, z; absolute voxel coordinates).
 * Free positions.  Position v of the region is free iff no voxel of the box [v, v + robot) blocks: iff se_hip_collide_boxes in
 *   SE_HIP_COLLIDE_STRICT mode answers a status > stop_at for (v, robot).  Classification, "outside the volume is unseen", "a pending index
 *   entry counts as absent" and the independence of how the tree happens to be subdivided are those of se_hip_collide_boxes.  The region may
 *   stick out of the volume or lie wholly outside it.
 * Moves.  From a free position to a free position of the region that differs by one voxel on one axis (6-connectivity).  Positions outside
 *   the region do not exist: the region's faces are walls.
 * Seeds.  A seed that lies outside the region, or whose position is not free, is ignored.  Seed coordinates are never refused: a seed
 *   anywhere in int32 is merely unusable.
 * Key.  steps(v) is the smallest number of moves from v to a usable seed, seed(v) the smallest seed index among the seeds at that distance,
 *   key(v) = steps(v) * 256 + seed(v).  key is the unique solution of: key(s_i) <= i for usable seeds, and key(v) = min(own seed index if
 *   any, min over free neighbours u of key(u) + 256).  Unreached positions have no key.
 * Outputs (se_hip_reach_out), each [side z][side y][side x]; steps is required, a null pointer for another array means "not wanted":
 *   steps   (int32) steps(v), or SE_HIP_REACH_NONE for a position that is not free or not connected to a usable seed.
 *   seed    (uint8) seed(v), or 255.
 *   next    (uint8) the first move of a shortest path to seed seed(v): the lowest direction code d whose neighbour u has key(u) + 256 ==
 *           key(v); codes 0 .. 5 are -x, +x, -y, +y, -z, +z; SE_HIP_REACH_AT_SEED where steps == 0; 255 where steps is NONE.  Following
 *           next from v reaches seed seed[v] after exactly steps[v] moves.
 *   counts  a HOST int64[4], in both entries: the number of free positions, the number of reached positions, the largest steps (-1 if
 *           nothing is reached), and the number of relaxation rounds the call ran.  Rounds are informational; rounds <= max steps + 2.
 * The whole call is refused with SE_HIP_E_INVALID, and then reads no map memory and writes nothing, for: a null request, test, out, steps or
 * seeds pointer; n_seeds outside 1 .. 255; a side or robot entry < 1; a robot entry > 256; any of lo, lo + side + robot outside
 * [-2^19, 2^19]; more than 2^24 positions; a stop_at, threshold or occupied_above that se_hip_distance_field refuses.
 * Work buffers in the handle's staging buffer: one bit per voxel of the block-aligned hull of the domain [lo, lo + side + robot - 1), three
 * bit arrays of at most that size, 4 bytes per position for the keys, two words per 32 x 8 x 8 tile.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream and a held-back raycast
 * included), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the map, the images and the launch counters
 * (SE_HIP_K_*) alone.
 * NEITHER ENTRY IS ASYNCHRONOUS.  The field is relaxed in rounds, one launch each, and the host decides after every round whether another is
 * needed: both entries have synchronised the handle's stream when they return.
 *   se_hip_reach_field       device output arrays (steps, seed, next); counts and seeds stay host pointers.
 *   se_hip_reach_field_host  host output arrays, staged through the same buffer. */
#define SE_HIP_REACH_NONE (-1)
#define SE_HIP_REACH_AT_SEED 6
#define SE_HIP_REACH_MAX_SEEDS 255
typedef struct se_hip_reach_request {
  int32_t lo[3];      /* x, y, z */
  int32_t side[3];
  int32_t robot[3];
  int32_t stop_at;
  int32_t n_seeds;
  const int32_t* seeds;  /* host: [n_seeds][3] */
} se_hip_reach_request;
typedef struct se_hip_reach_out {
  int32_t* steps;   /* [side z][side y][side x] */
  uint8_t* seed;
  uint8_t* next;
  int64_t* counts;  /* host: [4] */
} se_hip_reach_out;
int se_hip_reach_field(se_hip_pipeline* p, const se_hip_reach_request* request, const se_hip_collide_test* test,
                       const se_hip_reach_out* device_out);
int se_hip_reach_field_host(se_hip_pipeline* p, const se_hip_reach_request* request, const se_hip_collide_test* test,
                            const se_hip_reach_out* host_out);

/* ---- batched collision queries for oriented boxes: "does this robot, at this attitude, touch anything?" for N boxes at once, without
 *      getMap().  Not in the reference; built on its Octree::get and on the classification above.  The host restatement and the literal
 *      definition are include/se/oriented_collision.hpp.
 * Units: SE_HIP_ORIENTED_SUB = 16 sub-units per voxel.
 * Box: twelve int32, centre c xyz, then the half-axes h0, h1, h2 xyz, all in sub-units (boxes [n][12]).  The box is the open set
 *     { c + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1 }.
 *   The half-axes need not be orthogonal and may have either handedness: a rotation matrix rounded to fixed point is not exactly
 *   orthogonal, and the test does not need it to be.
 * Touched: take a cube with integer corner v and side s in voxels (a voxel: s = 1).  In doubled sub-units,
 *     m = 32 v + 16 s - 2 c   is the doubled offset from the box centre to the cube centre, and   e = 16 s   the doubled half-side of the cube.
 *   An integer axis a separates iff   a != 0   and   |a . m| >= 2 sum_i |a . h_i| + e sum_k |a_k|.
 *   The cube is touched iff none of these 15 axes separates: e_x, e_y, e_z, then h1 x h2, h2 x h0, h0 x h1, then h_i x e_k for the nine (i, k).
 *   The inequalities are open: a face, an edge or a vertex that only meets a voxel's boundary touches nothing.  The a != 0 clause is part of
 *   the definition: a half-axis parallel to a cube edge gives zero cross products, and without the clause 0 >= 0 would separate everything.
 *   For h_i = r_i e_i with c +- r on voxel boundaries the touched voxels are exactly those of the half-open box of SE_HIP_COLLIDE_STRICT.
 * Exactness: nothing is rounded.  With the bounds below and sizes up to 8192, a component of a cross product is a difference of two products
 *   of half-axis components: |a_k| <= 2 * 2^14 * 2^14 = 2^29, which fits int32.  |m_k| <= 32 * 8192 + 16 * 8192 + 2 * 2^20 < 2^22, so
 *   |a . m| <= 3 * 2^29 * 2^22 < 2^53.  On the right, sum_i |a . h_i| is |det(h0, h1, h2)| <= 6 * 2^42 for a face normal, at most
 *   2 * 2 * 2^28 = 2^30 for an edge cross product and 3 * 2^14 for a unit axis, and e sum_k |a_k| <= 2^17 * 3 * 2^29 < 2^47.6: every
 *   right-hand side stays below 2^49.  Everything is evaluated in int64.
 * A box is invalid if det(h0, h1, h2) == 0, if any |c_k| > 2^20, or if any |h_ik| > 2^14.  An invalid box gets status
 *   SE_HIP_COLLISION_INVALID and reads no map memory.
 * Status: the min over the touched voxels of classify(Octree::get(v)), exactly as in strict mode -- the voxel itself, or value_[child] of the
 *   deepest existing node; a pending index entry counts as absent; every voxel outside [0, size)^3 is unseen.  The box touches a voxel
 *   outside the volume iff, for some k, c_k - sum_i |h_ik| < 0 or c_k + sum_i |h_ik| > 16 size: no traversal is needed for that.  An absent
 *   touched octant folds classify(value_[child]), which is exact: an open set that meets an open cube meets the open cube of one of its voxels.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * boxes or status pointer with n > 0, a null test, a non-finite threshold and occupied_above other than 0 / 1 with SE_HIP_E_INVALID
 * (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the map, the images and the launch
 * counters (SE_HIP_K_*) alone.
 *   se_hip_collide_oriented       device arrays (boxes [n][12] int32, status [n] uint8); enqueued on the handle's stream, asynchronous like
 *                                 the stage calls.
 *   se_hip_collide_oriented_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_ORIENTED_SUB 16
#define SE_HIP_ORIENTED_CENTRE_LIMIT (1 << 20)
#define SE_HIP_ORIENTED_AXIS_LIMIT (1 << 14)
int se_hip_collide_oriented(se_hip_pipeline* p, const int32_t* device_boxes, int64_t n, const se_hip_collide_test* test, uint8_t* device_status);
int se_hip_collide_oriented_host(se_hip_pipeline* p, const int32_t* host_boxes, int64_t n, const se_hip_collide_test* test, uint8_t* host_status);

/* ---- batched collision queries for oriented boxes moved along straight segments: "may this robot, at this attitude, move from A to B, and
 *      if not, how far?" for N motions at once, without getMap().  se_hip_collide_motions for the box of se_hip_collide_oriented.  Not in the
 *      reference; built on its Octree::get and on the classification above.  The host restatement and the literal definition are
 *      include/se/oriented_motion.hpp.
 * Units: SE_HIP_ORIENTED_SUB = 16 sub-units per voxel.
 * Motion: fifteen int32, centre c xyz, half-axes h0, h1, h2 xyz, displacement d xyz (motions [n][15]).  At parameter t in [0, 1] the box is the
 *   open set   B(t) = { c + t d + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1 }.   The half-axes need not be orthogonal, as for the static query; the
 *   attitude does not change during the motion.
 * Touched: a cube with integer corner v and side s in voxels (a voxel: s = 1) is touched iff some t in [0, 1] has B(t) touching it in the
 *   sense of se_hip_collide_oriented.  Written out, with the fifteen axes of that query (e_k, h_i x h_j, h_i x e_k; a zero axis takes no
 *   part), per axis a:
 *     m = 32 v + 16 s - 2 c,   p = a . m,   q = 2 (a . d),   R = 2 sum_i |a . h_i| + 16 s sum_k |a_k|.
 *   The box at t is not separated by a iff |p - t q| < R.  An axis with q = 0 gives the static condition |p| < R; every other axis the open
 *   interval ((p' - R) / |q|, (p' + R) / |q|) with p' = p sign(q).  With L the largest lower end and U the smallest upper end over those axes
 *   (L = 0, U = 1 when there is none) the cube is touched iff every static condition holds and L < U, L < 1, U > 0, and its entry parameter
 *   is t_in = max(0, L).  All inequalities are open.  t_in is an infimum: a box whose vertex only meets a voxel's corner at t = 0 and then
 *   slides into the voxel has t_in = 0, although the static query at t = 0 says "not touched".
 * Equivalent form (used for pruning and for the touched test on the device; the host tests hold the two together): the swept set is the open
 *   zonotope with generators h0, h1, h2, d / 2 about c + d / 2, and a cube is touched iff none of the 21 axes e_k, g_i x g_j, g_i x e_k with
 *   g = (h0, h1, h2, d) separates; an axis a != 0 separates iff
 *     |a . (32 v + 16 s - 2 c - d)| >= 2 sum_i |a . h_i| + |a . d| + 16 s sum_k |a_k|.
 * A motion is invalid if its box is invalid for se_hip_collide_oriented (det(h0, h1, h2) == 0, |c_k| > 2^20, |h_ik| > 2^14), if any
 *   |d_k| > SE_HIP_ORIENTED_MOVE_LIMIT = 2^18 (16 384 voxels, twice the largest volume) or if any |c_k + d_k| > 2^20.  An invalid motion gets
 *   status SE_HIP_COLLISION_INVALID, t_first = -1, t_exact = (-1, 1), and reads no map memory.
 * Exactness: nothing is rounded before the final conversion.  With those bounds and sizes up to 8192, for the fifteen axes |a_k| <= 2^29 as
 *   in the static query, |m_k| < 2^22 and |p| <= 3 * 2^29 * 2^22 < 2^53; |q| <= 2 * 3 * 2^29 * 2^18 < 2^50; R < 2^49 as there: the numerators
 *   p' +- R stay below 2^54.  A component of h_i x d or d x e_k is at most 2 * 2^14 * 2^18 = 2^33; |32 v + 16 s - 2 c - d| < 2^22 + 2^18, so
 *   the left side of the 21-axis form is below 3 * 2^33 * 2^22.1 < 2^57, and on its right 2 sum_i |a . h_i| <= 2 * 3 * 3 * 2^33 * 2^14 < 2^52
 *   and 16 s sum_k |a_k| <= 2^17 * 3 * 2^33 < 2^52: both sides stay below 2^59.  Everything is int64 except the comparison of two rationals,
 *   which is a cross-multiplication in 128 bits (products below 2^104); there is no 128-bit division.
 * Classification: exactly that of se_hip_collide_oriented and of SE_HIP_COLLIDE_STRICT -- `test` applied to Octree::get(v), a pending index
 *   entry counts as absent, voxels outside [0, size)^3 are unseen.  The box touches a voxel outside the volume at t iff, for some k,
 *   c_k + t d_k - ext_k < 0 or c_k + t d_k + ext_k > 16 size with ext_k = sum_i |h_ik|: the outside's contribution to status, and to the
 *   entry parameter when stop_at is unseen, is closed form per face.  An absent touched octant folds classify(value_[child]), and the octant's
 *   own t_in when that class blocks; both are exact by the open-set argument of the static query.
 * Outputs (se_hip_oriented_motion_out; status is required, a null t_first or t_exact means "not wanted"):
 *   status[n]      (uint8) the min class over the touched voxels, as for se_hip_collide_motions.
 *   t_exact[n][2]  (int64) with stop_at in {SE_HIP_COLLISION_OCCUPIED, SE_HIP_COLLISION_UNSEEN}, a voxel blocks when its class is <= stop_at;
 *                  the smallest t_in over the touched blocking voxels (those outside the volume included) as a reduced fraction num / den,
 *                  den > 0, gcd = 1: (0, 1) when blocked from the start, (2, 1) when nothing blocks, (-1, 1) for an invalid motion.
 *   t_first[n]     (float) (float)((double)num / (double)den) of that reduced pair -- reduced first, so that the float depends on the value
 *                  only; SE_HIP_MOTION_FREE (2.0f) when nothing blocks, -1.0f for an invalid motion.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * out, a null motions or status pointer with n > 0, a null test, a non-finite threshold, occupied_above other than 0 / 1 and a stop_at other
 * than the two above with SE_HIP_E_INVALID (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the
 * map, the images and the launch counters (SE_HIP_K_*) alone.
 *   se_hip_collide_oriented_motions       device arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_collide_oriented_motions_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it
 *                                         returns. */
#define SE_HIP_ORIENTED_MOVE_LIMIT (1 << 18)
typedef struct se_hip_oriented_motion_out {
  uint8_t* status;   /* [n] */
  float* t_first;    /* [n] */
  int64_t* t_exact;  /* [n][2] */
} se_hip_oriented_motion_out;
int se_hip_collide_oriented_motions(se_hip_pipeline* p, const int32_t* device_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                                    const se_hip_oriented_motion_out* device_out);
int se_hip_collide_oriented_motions_host(se_hip_pipeline* p, const int32_t* host_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                                         const se_hip_oriented_motion_out* host_out);

/* ---- exact segment traces: "is there a free line of sight from A to B, and if not, which voxel is in the way?" and "how much unseen space
 *      would a sensor at this pose look into?" for N segments at once, without getMap().  The motion query for a point, in traversal order,
 *      with class counts: the occupancy-reader counterpart of se_hip_cast_rays, which marches the float field through allocated blocks only
 *      and does not know the three classes.  Not in the reference; built on its Octree::get and on the classification above.  The host
 *      restatement and the literal definition are include/se/segment_trace.hpp.
 * Units: SE_HIP_ORIENTED_SUB = 16 sub-units per voxel, the same as the oriented boxes.
 * Segment: six int32, a xyz, b xyz in sub-units (segments [n][6]).  Let d = b - a and P(t) = a + t d for t in [0, 1].
 * Touched: a cube with integer corner c and side s (a voxel: s = 1) is touched iff some t in [0, 1] has, on every axis k,
 *     16 c_k < a_k + t d_k < 16 (c_k + s).
 *   This is se_hip_collide_motions' rule for a box of side 0, in sub-units; the inequalities are open.  An axis with d_k = 0 gives a static
 *   condition, every other axis an open interval with rational ends over |d_k|; with L the largest lower end and U the smallest upper end the
 *   cube is touched iff L < U, L < 1 and U > 0, and a touched voxel's entry parameter is t_in = max(0, L).
 *   - A segment that has d_k = 0 and a_k = 0 (mod 16) on some axis lies in a grid plane: it touches nothing, and that is a valid answer.
 *   - A segment through a voxel edge or corner passes diagonally: the voxels that share only that edge or corner are not touched.
 *   - The touched voxels of one segment have pairwise distinct t_in, so the order by t_in is the order of traversal.
 *   Every comparison is exact (cross-multiplication in int64): nothing depends on a step or a rounding.
 * Classification: exactly that of se_hip_collide_boxes in strict mode -- `test` applied to Octree::get(v) (the voxel, or value_[child] of the
 *   deepest existing node; a pending index entry counts as absent); every voxel outside [0, size)^3 is unseen.  With stop_at in
 *   {SE_HIP_COLLISION_OCCUPIED, SE_HIP_COLLISION_UNSEEN}, a voxel blocks when its class is <= stop_at, as in se_hip_collide_motions.
 * A segment with any coordinate of a or b outside [-2^22, 2^22] (SE_HIP_SEGMENT_LIMIT) is invalid and reads no map memory.  (The bound keeps
 *   every numerator and denominator at or below 2^23 -- exactly representable as floats --, every cross product below 2^47 and every position
 *   numerator a_j den + num d_j below 2^47: everything fits int64.)
 * Outputs (se_hip_trace_out; status is required, a null pointer for another array means "not wanted"):
 *   status[n]     (uint8) the min class over the touched voxels up to and including the first blocking voxel -- over all touched voxels when
 *                 nothing blocks; SE_HIP_COLLISION_EMPTY when nothing is touched; SE_HIP_COLLISION_INVALID for an invalid segment.
 *   t_first[n]    (float) t_in of the first blocking voxel in traversal order, voxels outside the volume included, returned as
 *                 (float)num / (float)den of the exact rational, as in se_hip_collide_motions; SE_HIP_MOTION_FREE (2.0f) when nothing blocks,
 *                 -1.0f for an invalid segment.
 *   first[n][3]   (int32, x y z) that voxel; three times INT32_MIN when nothing blocks or the segment is invalid.
 *   counts[n][2]  (int32) the number of unseen voxels and of empty voxels among the touched voxels inside the volume that precede the first
 *                 blocking voxel -- all touched voxels inside the volume when nothing blocks; (-1, -1) for an invalid segment.  Voxels outside
 *                 the volume are never counted (there is nothing to learn there); they do block under stop_at unseen.  With stop_at occupied,
 *                 counts[.][0] is the information gain of the ray; with stop_at unseen it is 0 and counts[.][1] is the free run.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * out, a null segments or status pointer with n > 0, a null test, a non-finite threshold, occupied_above other than 0 / 1 and a stop_at other
 * than the two above with SE_HIP_E_INVALID (n == 0 is a no-op), report a sticky SE_HIP_E_CAPACITY like the other read-back calls, and leave the
 * map, the images, the image ring, the launch counters (SE_HIP_K_*) and the timing sums alone.
 *   se_hip_trace_segments       device arrays; one launch enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_trace_segments_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_SEGMENT_LIMIT (1 << 22)
typedef struct se_hip_trace_out {
  uint8_t* status;  /* [n]    */
  float* t_first;   /* [n]    */
  int32_t* first;   /* [n][3] */
  int32_t* counts;  /* [n][2] */
} se_hip_trace_out;
int se_hip_trace_segments(se_hip_pipeline* p, const int32_t* device_segments, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                          const se_hip_trace_out* device_out);
int se_hip_trace_segments_host(se_hip_pipeline* p, const int32_t* host_segments, int64_t n, const se_hip_collide_test* test, int32_t stop_at,
                               const se_hip_trace_out* host_out);

/* ---- batched ray casts against the resident map: the per-pixel body of the reference's raycastKernel (se_denseslam/src/rendering.cpp:51-90)
 *      for N rays of the caller's at once, without getMap() -- simulated range sensors, line-of-sight checks, views from poses that are not
 *      the tracked camera's.
 * Ray: 8 floats, ox oy oz dx dy dz near far, in metres in the world frame (rays [n][8] float32).  For each ray, with o, d, near, far in place
 *   of the camera's origin, pixel direction and planes:
 *     1. the ray iterator (ray_iterator.hpp) over the map index from o along d within [near, far]: ray.next(), then t_min = ray.tcmin();
 *     2. if t_min > 0: hit = raycast(volume, o, d, t_min, ray.tmax(), mu, step, largestep), the field's march (kfusion for SDF, bfusion
 *        for OFusion), step = dim / size, largestep = 8 * step (as the camera raycast sets them);
 *     3. if hit.w > 0: normal = normalized(-grad(hit)) for SDF, normalized(+grad(hit)) for OFusion (Octree::grad, scaled by 0.5 * dim / size);
 *        a zero gradient gives INVALID (-2, 0, 0).
 *   d is used as given: it is not normalised on the device, so a caller who normalised it in float (as the camera does, f3_normalized) gets
 *   the camera raycast's bits.  near > far and near <= 0 are not refused: they take whatever the reference does (t_min clamping, then the
 *   t_min > 0 test).  There is no frame gate (the camera path's frame > 2 does not apply).
 * Outputs (a null pointer means "not wanted"; at least one must be set):
 *   hit[n][4]     x y z t: the V4f raycast returns, {0, 0, 0, 0} when it finds no crossing (and for a ray that does not reach step 2);
 *   normal[n][3]  as in step 3; (-2, 0, 0) without a hit;
 *   status[n]     (uint8) bit 0 (1) VALID: the ray passed the checks below; bit 1 (2) ENTERED: the iterator returned an allocated block at
 *                 t_min > 0, the march ran; bit 2 (4) HIT: hit.w > 0; bit 3 (8) NORMAL: the gradient at the hit is not zero.
 * Defined beyond the reference -- INVALID rays: status 0, hit {0, 0, 0, 0}, normal (-2, 0, 0), no map memory read:
 *   - any non-finite value among the 8 floats;
 *   - |s * o| >= 2^20 on any axis, s = (float)size / dim (the limit of se_hip_query_points);
 *   - a direction whose squared norm (dx * dx + dy * dy) + dz * dz lies outside [0.98, 1.02] (float arithmetic, no FMA).  The band bounds
 *     the march: a near-zero direction would mean an effectively unbounded number of steps for one ray.
 * mu (kfusion's march uses it; one value per call) must be finite and > 0.  The first-leaf search stops after 4096 trips, as the camera
 * raycast's does.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), refuse n < 0, a null
 * rays pointer with n > 0, no output or a bad mu with SE_HIP_E_INVALID (n == 0 is a no-op), and report a sticky SE_HIP_E_CAPACITY like the
 * other read-back calls.  They leave the map, the vertex / normal images and the image ring, a deferred raycast (not launched by them), the
 * launch counters (SE_HIP_K_*) and the timing sums alone.
 *   se_hip_cast_rays       device arrays; enqueued on the handle's stream, asynchronous like the stage calls (batches beyond 2^24 rays are
 *                          split into several launches).
 *   se_hip_cast_rays_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_RAY_VALID 1
#define SE_HIP_RAY_ENTERED 2
#define SE_HIP_RAY_HIT 4
#define SE_HIP_RAY_NORMAL 8
typedef struct se_hip_ray_out {
  float* hit;       /* [n][4] */
  float* normal;    /* [n][3] */
  uint8_t* status;  /* [n]    */
} se_hip_ray_out;
int se_hip_cast_rays(se_hip_pipeline* p, const float* device_rays, int64_t n, float mu, const se_hip_ray_out* device_out);
int se_hip_cast_rays_host(se_hip_pipeline* p, const float* host_rays, int64_t n, float mu, const se_hip_ray_out* host_out);

/* ---- "next" row f-4: Octree::save (se_core/include/se/octree.hpp:898-914, io/se_serialise.hpp:54-86),
 *      written straight from the device map in the reference's byte layout:
 *        int32 size, float dim, uint64 n_nodes, n_nodes x {uint64 code, int32 side, value_[8]},
 *        uint64 n_blocks, n_blocks x {uint64 code, int32 coords[3], voxel_block_[512]}
 *      with value_type = {float x, float y} (SDF) or {float x, 4 pad bytes, double y} (OFusion).
 *      Nodes and blocks are written sorted by key (the reference writes its pool order, which is
 *      nondeterministic under OpenMP). */
int se_hip_save_map(se_hip_pipeline* p, const char* filename);
/* Octree::load (se_core/include/se/octree.hpp:917-950): re-initialises the device map and restores it from a file in
 * the layout above (written by se_hip_save_map or by the reference's Octree::save) for the same size / dim / field
 * type.  The reference's load() reads `dim` as an int and restores one voxel per block (octree.hpp:921-924, 945-946);
 * this one reads the float and restores all 512.  Blocks come back active, as Octree::insert leaves them. */
int se_hip_load_map(se_hip_pipeline* p, const char* filename);

/* ---- rolling volume: the map content translated by a whole number of blocks, on the device (no reference counterpart: the reference's volume is
 *      a fixed cube and nothing in it is ever freed).  The executable definition is se::shift_map of include/se/shift_map.hpp on the getMap()
 *      snapshot.  s = shift_voxels: content at voxel c before the call is at c + s after it; what leaves the cube is forgotten, the vacated side
 *      is unseen.  A robot that walks towards +x passes a negative s[0].
 *        arguments  every component a multiple of 8 (the block side) within [-2^30, 2^30], else SE_HIP_E_INVALID and the map is untouched
 *                   (as with every other entry, a raycast that was held back has been launched by then: the images may have advanced);
 *                   s = 0 is valid and changes nothing
 *        blocks     the block with corner c survives iff c + s lies in [0, size - 8] on every axis; it keeps its 512 x and y values bit for bit
 *                   and its active flag
 *        nodes      the node with side d and corner c survives iff every component of s is a multiple of d and c + s lies in [0, size - d]; it
 *                   keeps value_[8].  A node the shift is not aligned to is dropped (its children would no longer be its children).  The root
 *                   always exists afterwards and keeps its values only for s = 0
 *        closure    every missing ancestor of a survivor is created with initValue(), as Octree::allocate creates it (without the keys[0] rule of
 *                   unique_multiscale); nothing else exists afterwards; surviving childless nodes stay
 *        counts     (optional, host, int64[4]) blocks kept, blocks dropped, nodes kept, nodes dropped (the root counts as kept only for s = 0);
 *                   the nodes created follow from se_hip_counts
 *        pools      dense grid: every vacated brick and every dropped block's brick reads initValue() again.  Pooled: the pools are compact
 *                   afterwards (used slots = survivors), every free slot holds initValue()
 *      Everything derived from the block set -- index, occupancy and beam-start bitmaps, lists, counters -- is rebuilt for the new set; the
 *      count words of the new-key lists and the statistics counters of se_hip_get_stats are zeroed, as se_hip_load_map zeroes them.  A deferred
 *      raycast is launched first (it belongs to the old frame of reference), a scan on the side stream is joined, and the call returns when the
 *      map is shifted (it synchronises the handle, as se_hip_load_map does).  The work is per block, not per cell of the volume; the survivors
 *      pass through a staging buffer of 4 KiB per block, which is released again when it is larger than 64 MiB.
 *      vertex_ / normal_ are not touched: they stay in the frame of reference before the shift, and after a nonzero shift se_hip_track and
 *      se_hip_frame_tracked return SE_HIP_E_INVALID ("vertex / normal images predate a map shift") until a raycast has run; se_hip_render_volume
 *      casts its own rays until then.  Poses are the caller's: after the call it passes poses translated by s * dim / size.
 *      A node pool that runs out while the ancestors are rebuilt raises the usual sticky SE_HIP_E_CAPACITY.  Replicas (row-sharded,
 *      sharded sweep) each hold the whole map: the same call goes to every one of them.
 *      Between the scan and the sweep of a frame (se_hip_alloc_scan ... se_hip_integrate_sweep) the call is allowed: the scan is joined, so the
 *      blocks it inserted exist, are active and move with the map like any other; their occupancy bits and beam-start marks come from the
 *      rebuild above, and the sweep owes the scan no commit any more.  The sweep that follows takes the pose
 *      the caller passes -- translated by s * dim / size -- and integrates the frame into the shifted map (tests/test_gpu_op_programs.py,
 *      program staged_shift_merge, against the oracle). */
int se_hip_shift_map(se_hip_pipeline* p, const int32_t shift_voxels[3], int64_t* host_counts);

/* ---- release: octants that lie wholly inside a box handed back on the device -- all of them (the region is forgotten) or only those that hold
 *      nothing (no reference counterpart: nothing in the reference's octree is ever freed).  The executable definition is se::release_map of
 *      include/se/release_map.hpp on the getMap() snapshot.
 *        arguments  host records; 0 <= n <= 4096; per record the box is [lo, lo + side) per axis, in voxels, side >= 1, lo and lo + side within
 *                   [-2^30, 2^30], what one of the two codes, reserved 0; a null host_boxes with n > 0 or anything else: SE_HIP_E_INVALID and the
 *                   map is untouched (as with every other entry, a raycast that was held back has been launched by then).  Boxes need not be
 *                   multiples of 8: a record contains the octant with corner c and side d iff c >= lo and c + d <= lo + side on every axis
 *                   (partial forgetting is se_hip_edit_boxes' reset).  n = 0 is valid, changes nothing and returns the counts of the map as it is
 *        blocks     released iff some record contains the block and that record is ALL, or is UNSEEN and all 512 voxels equal initValue() in x
 *                   and y bit for bit, as se_hip_download_blocks returns them (the SDF weight byte converted to float)
 *        nodes      releasable iff some record contains the node and that record is ALL or all eight value_[i] equal initValue() bit for bit;
 *                   released iff releasable and every block and node beneath it is released.  The root always stays.  An ancestor of a
 *                   survivor is never released: nothing is created
 *        parents    for every released octant whose parent stays, the parent's value_[child] becomes initValue().  Nothing else in a survivor
 *                   changes: 512 values, value_[8] and the active flag bit for bit.  So Octree::get(v) is initValue() for every voxel of a released
 *                   block: a call with UNSEEN records only changes the answer of get at no voxel and the strict status of no box; an ALL
 *                   record turns its blocks unseen
 *        counts     (optional, host, int64[5]) blocks kept, blocks released, nodes kept (the root included), nodes released, released blocks
 *                   that held at least one observed voxel
 *        touched    (optional, host, int32[6]) lo[3] and hi[3] of the voxel box that holds every released block (half open, as se_hip_merge_map
 *                   reports its box; all zero if none)
 *      A call that releases nothing changes nothing: no rebuild, no pool compaction.  Otherwise everything derived from the block set -- index,
 *      occupancy and beam-start bitmaps, lists, counters -- is rebuilt for the survivors as se_hip_shift_map rebuilds it: the pools are compact
 *      afterwards (used slots = survivors), every free slot and every vacated dense brick reads initValue(), the count words of the new-key
 *      lists and the statistics counters of se_hip_get_stats are zeroed.  A held-back raycast is launched first, a scan on the side stream is
 *      joined, and the call returns synchronised.  The work is per block and per record, not per cell of the volume; the survivors pass through
 *      the shift's staging (4 KiB per block, released again when it is larger than 64 MiB).  No pool can run out: nothing is created.
 *      vertex_ / normal_ stay valid (the frame of reference did not move: tracking goes on).  Replicas each hold the whole map: the same call
 *      goes to every one of them.  Between the scan and the sweep of a frame (se_hip_alloc_scan ... se_hip_integrate_sweep) the call is
 *      allowed: it acts on the state after the join, where the scan's fresh blocks are ordinary all-unseen blocks, and the sweep owes the scan
 *      no commit any more.  A block that holds nothing but is still in view and inside the allocation band is created again by the next
 *      allocation scan: the lasting gain is in regions the camera has left, before a save or a merge, and under a pooled budget. */
#define SE_HIP_RELEASE_ALL    1   /* every octant wholly inside the box: the region is forgotten */
#define SE_HIP_RELEASE_UNSEEN 2   /* only octants that hold nothing */
#define SE_HIP_RELEASE_MAX_BOXES 4096
typedef struct se_hip_release_box { int32_t lo[3]; int32_t side[3]; int32_t what; int32_t reserved; } se_hip_release_box;
int se_hip_release_boxes(se_hip_pipeline* p, const se_hip_release_box* host_boxes, int64_t n,
                         int64_t* host_counts /* [5], optional */, int32_t* host_touched /* lo xyz, hi xyz, optional */);

/* ---- map merge: the content of one resident map (src) folded into another (dst) on the device, optionally moved by a whole number of blocks (no
 *      reference counterpart: the reference holds one map).  The executable definition is se::merge_map / se::merge_value of
 *      include/se/merge_map.hpp on two getMap() snapshots.  s = shift_voxels: source content at voxel c meets destination content at c + s.
 *        arguments  SE_HIP_E_INVALID, both maps untouched (a held-back raycast of either handle may have been launched by then): dst == src; different
 *                   devices; different field types; different voxel size (dim / size, a binary32 division, not bit-equal); a component of s that is
 *                   not a multiple of 8 or lies outside [-2^30, 2^30]; a null rule, an unknown mode, a max_weight that is not an integer in
 *                   [1, 255] (checked for both field types, used by SDF only).  The volume sizes may differ.  A source with a sticky
 *                   SE_HIP_E_CAPACITY is refused with that code: it is not the map the reference would hold
 *        unseen     a value v with v.x == initValue().x && v.y == initValue().y (y compared as float), as the collision queries mean it
 *        values     a = destination value, b = source value, for block voxels and node value_[j] alike:
 *                     b unseen                   a stays, bit for bit, in every mode
 *                     a unseen, or REPLACE       b, bit for bit; SDF: y = fminf(b.y, max_weight)
 *                     FILL                       a stays
 *                     FUSE, SDF                  b.y == 0: a stays; a.y == 0: as "a unseen"; else w = a.y + b.y,
 *                                                x = clamp((a.y * a.x + b.y * b.x) / w, -1, 1), y = fminf(w, max_weight) -- sdf_update's running mean with the
 *                                                second sample weighing b.y instead of 1; binary32 in that order, no contraction, IEEE division; the
 *                                                weights are added as floats, never as bytes (200 + 100 gives max_weight)
 *                     FUSE, OFusion              x = clamp(a.x + b.x, -1000, 1000) (BOTTOM_CLAMP, TOP_CLAMP of volume_traits.hpp: the prior is log-odds 0,
 *                                                independent evidence adds), y = fmaxf(a.y, b.y)
 *                   clamp(v, lo, hi) = std::max(lo, std::min(v, hi)), as everywhere in the library
 *        blocks     the source block with corner c takes part iff c + s lies in [0, dst size - 8] on every axis, else it is clipped.  Its block in dst
 *                   is created if absent, with all missing ancestors and initValue() (Octree::allocate, without the keys[0] rule); the 512 values are
 *                   combined; active = the OR of the two flags, a created block is active, as insertion leaves it
 *        nodes      the source node of side d (level >= 1, childless ones included) and corner c takes part iff every component of s is a multiple
 *                   of d and c + s lies in [0, dst size - d]; its level is the one of side d in dst.  It is created if absent and its value_[8] are
 *                   combined.  Any other source node contributes nothing (skipped).  The source root takes part only if s == 0 and the sizes are
 *                   equal.  Coarse values meet coarse values only: a source node value is never pushed down into destination voxels
 *        counts     (optional, host, int64[12]) blocks combined into existing blocks, blocks created, source blocks clipped, nodes combined into
 *                   existing nodes, nodes created for source nodes, source nodes skipped, lo[3] and hi[3] of the destination voxel box that holds
 *                   every block that took part (half open; all zero if none).  Ancestors created on the way follow from se_hip_counts
 *      On both handles a held-back raycast is launched first and a scan on the side stream is joined; both are synchronised before the first kernel,
 *      which runs on dst's stream, and the call returns synchronised.  src is only read.  dst's vertex_ / normal_ stay valid (its frame of reference
 *      did not move: tracking goes on).  A destination pool that runs out raises the usual sticky SE_HIP_E_CAPACITY; a source block whose
 *      destination found no slot is skipped.  No launch counter and no timing sum changes.  The staging is 12 bytes per source block and node.
 *      Replicas each hold the whole map: the same call goes to every one of them.  Across devices: save, load into a scratch handle, merge.
 *      Between the scan and the sweep of a frame (se_hip_alloc_scan ... se_hip_integrate_sweep), on dst or on src, the call is allowed: the scan is
 *      joined, so the blocks it inserted take part like any other (on dst they are combined with, on src they are merged from, holding
 *      initValue()); joining publishes the occupancy bits and beam-start marks of the scan's keys at once (as every entry point does that joins
 *      a scan), the merge inserts its own blocks in place, and the sweep that follows owes the scan nothing and integrates the frame into the
 *      merged map (same test: program staged_shift_merge for dst, test_a_merge_from_a_source_between_its_scan_and_its_sweep for src). */
#define SE_HIP_MERGE_FUSE    0   /* both observed: combine */
#define SE_HIP_MERGE_REPLACE 1   /* source wins wherever the source is observed */
#define SE_HIP_MERGE_FILL    2   /* destination wins; source only where destination is unseen */
typedef struct se_hip_merge_rule { int32_t mode; float max_weight; /* SDF only; integer in [1, 255]; mirrors default to 100 */ } se_hip_merge_rule;
int se_hip_merge_map(se_hip_pipeline* dst, se_hip_pipeline* src, const int32_t shift_voxels[3],
                     const se_hip_merge_rule* rule, int64_t* host_counts /* optional, [12] */);

/* ---- map merge under a rigid transform: the content of src resampled into dst's lattice under a rotation and any translation, then combined with
 *      the same value-pair rule (no reference counterpart).  The executable definition is se::rigid_sample / se::merge_map_rigid of
 *      include/se/merge_rigid.hpp on two getMap() snapshots.  src_from_dst is the PULL transform, row-major 3 x 4, in voxels: R = its first
 *      three columns, t = the fourth.  The call never inverts it, so the result is exact for the twelve floats passed (the mirrors build them from
 *      a metric pose: rigid_pull / rigidPull).
 *        convention a voxel with integer coordinates v holds the field at position v, in voxels (the library's interp convention: the cell's lower
 *                   corner is floor(q)); there is no half-voxel offset
 *        position   for a destination voxel v: q_k = ((R_k0 * vx + R_k1 * vy) + R_k2 * vz) + t_k, binary32 in that order, no contraction;
 *                   l = floor(q), f = q - floorf(q)
 *        validity   the sample is valid iff 0 <= l_k and l_k + 1 <= src size - 1 on every axis and none of the eight corner voxels l + {0,1}^3 is
 *                   unseen.  Corners are read as get_fine reads them (initValue() where the source has no block); "unseen" as above.  A cell with
 *                   any unseen corner contributes nothing: no extrapolation, no empty() substitution
 *        value      b.x = the trilinear blend of the corner x values p[i + 2j + 4k] in Octree::interp's term order,
 *                     ((p0 (1-fx) + p1 fx) (1-fy) + (p2 (1-fx) + p3 fx) fy) (1-fz) + ((p4 (1-fx) + p5 fx) (1-fy) + (p6 (1-fx) + p7 fx) fy) fz;
 *                   SDF: b.y = the minimum of the eight corner weights (an integer in 0 .. 255); OFusion: b.y = the maximum of the eight corner
 *                   times.  The sample is observed iff it is valid and b itself is not unseen
 *        values     every destination voxel with an observed sample becomes merge_value(a, b, mode, max_weight), the table above; every other
 *                   voxel keeps its bits
 *        blocks     an absent destination block is created iff at least one of its 512 voxels has an observed sample, with all missing ancestors
 *                   and initValue() (without the keys[0] rule); no other block is created.  Every destination block that receives at least one
 *                   observed sample is active afterwards, as insertion leaves a new block
 *        nodes      source node values never take part (coarse values cannot be resampled); destination node values are untouched; ancestors
 *                   created on the way hold initValue()
 *        counts     (optional, host, int64[10]) blocks that existed and received an observed sample, blocks created, voxels with an observed
 *                   sample, of those the voxels whose destination value was observed before, lo[3] and hi[3] of the half-open destination voxel
 *                   box over the blocks that received samples (all zero if none)
 *        arguments  SE_HIP_E_INVALID, both maps untouched: everything se_hip_merge_map refuses (dst == src, devices, field types, voxel sizes,
 *                   the rule); a null transform or a non-finite entry; |t_k| > 2^20; max |R^T R - I| > 1e-3 or det R <= 0, both evaluated in
 *                   double (the transform must be rigid: no scale, no mirror; a binary32 rotation from a normalised quaternion is off by about
 *                   1e-6).  A source with a sticky SE_HIP_E_CAPACITY is refused with that code
 *      Non-finite source values: the library never produces them; the result for them is unspecified.
 *      Schedule, pool exhaustion and staging ownership are those of se_hip_merge_map: a held-back raycast of either handle is launched first,
 *      scans are joined, all streams are synchronised before the first kernel, which runs on dst's stream, and the call returns synchronised;
 *      a destination pool that runs out raises the sticky SE_HIP_E_CAPACITY and a block that found no slot is skipped; dst's images stay valid
 *      and tracking goes on; no launch counter or timing sum moves.  The staging (dst's) is one bit per destination block plus 12 bytes per
 *      candidate block (at most 64 per source block, at most the destination's block grid). */
int se_hip_merge_map_rigid(se_hip_pipeline* dst, se_hip_pipeline* src, const float src_from_dst[12],
                           const se_hip_merge_rule* rule, int64_t* host_counts /* optional, [10] */);

/* ---- map export, second half: marching cubes over the allocated blocks
 * DenseSLAMSystem::dump_mesh (DenseSLAMSystem.cpp:302-322) = se::algorithms::marching_cube
 * (se_core/include/se/algorithms/meshing.hpp:161-208) with inside(v) = v.x < 0, select(v) = v.x, then writeVtkMesh
 * (se_denseslam/include/se/commons.h:325-390).  Vertices (which cell edges carry one, and where) are the
 * reference's, and so is the split of a cell's polygon into triangles: include/se_mc_table.h is the standard marching-cubes
 * table, content-identical to the reference's edge_tables.h:66 (tests/test_mc_table_reference.py).  A triangle is 9 floats (3 vertices, metres); their order is unspecified, as in the
 * reference (OpenMP completion order there). */
int se_hip_mesh_count(se_hip_pipeline* p, int64_t* n_triangles);
int se_hip_mesh_download(se_hip_pipeline* p, float* host_triangles, int64_t capacity_triangles, int64_t* n_written);
/* dump_mesh(filename): ASCII VTK polydata in writeVtkMesh's format, triangles sorted for reproducibility */
int se_hip_dump_mesh(se_hip_pipeline* p, const char* filename);

/* ---- live meshing: the triangles of the blocks that a region and a set of views select, grouped per block
 * The same cells, vertices and triangles as se_hip_mesh_download, produced in one pass on the handle's stream, for a viewer or a mesh
 * publisher that replaces exactly the blocks that may have changed.
 * Selection (se_hip_mesh_select, host memory, read before the call returns):
 *   lo, hi    a half-open box in voxels.  A block is in the region if its 8^3 voxels intersect it; lo = 0, hi = size is the whole volume.
 *             Coordinates outside the volume are clamped; an empty or inverted box selects nothing.
 *   n_views   0 .. SE_HIP_MESH_MAX_VIEWS.  0: the region alone decides.  Otherwise a block must also be possibly touched by at least one of
 *   views[]   the views: camera-to-world pose (column-major, as the stage calls take it), k = fx fy cx cy, image width and height.  The test
 *             is conservative -- a superset of the blocks with a voxel of their 9^3 dependency box (own voxels plus the +1 layer the cells
 *             read) that integration would update under that view: the box's bounding sphere (centre 8 b + 4, radius rounded up to 9
 *             voxels) against the half space z > 0 and the four side planes through pixel columns -1 and width, rows -1 and height.
 *             fx or fy may be negative.
 *   flags     SE_HIP_MESH_SKIP_EMPTY: selected blocks without a triangle are left out of the table (default: listed with count 0, so that a
 *             receiver can delete a block whose surface has gone).
 * Output (se_hip_mesh_out; device pointers for se_hip_mesh_blocks, host pointers for se_hip_mesh_blocks_host):
 *   triangles[capacity_triangles][9]  floats, metres;
 *   block_coords[capacity_blocks][3]  voxel coordinates of the block's corner; block_range[capacity_blocks][2]  first, count into triangles;
 *   header[4]  blocks listed (the table size needed), triangles needed, blocks written, triangles written.
 * Only whole blocks are written: the table rows [0, header[2]) and the triangles [0, header[3]), ranges disjoint and without gaps.  When a
 * capacity is too small, header[0] and header[1] still give the sizes needed.  triangles == NULL with both capacities 0 is the sizing call.
 * The order of the table's rows is unspecified.  Within a block the order is defined: cells x fastest, then y, then z, a cell's triangles
 * in table order -- a block's payload is a function of the map alone.
 * Both entries answer for the map after everything enqueued before them (a scan that ran on the side stream included), and leave the map,
 * the images and the image ring, a deferred raycast, the launch counters and the timing sums alone.  They refuse null pointers where one
 * is needed (header; triangles / the block arrays with a capacity > 0; views with n_views > 0), negative capacities, n_views out of range,
 * unknown flags, non-finite view values, fx or fy == 0 and non-positive image sizes with SE_HIP_E_INVALID before any launch.
 *   se_hip_mesh_blocks       asynchronous on the handle's stream; no synchronisation, no allocation per call; on overflow the header tells.
 *   se_hip_mesh_blocks_host  staged through a device buffer the handle keeps (and grows); synchronises; SE_HIP_E_CAPACITY after filling
 *                            what fitted (the sizing call returns SE_HIP_OK). */
#define SE_HIP_MESH_MAX_VIEWS 64
#define SE_HIP_MESH_SKIP_EMPTY 1u
typedef struct se_hip_mesh_view {
  float pose[16];   /* camera -> world, column-major */
  float k[4];       /* fx, fy, cx, cy */
  int32_t width, height;
} se_hip_mesh_view;
typedef struct se_hip_mesh_select {
  int32_t lo[3], hi[3];
  int32_t n_views;
  uint32_t flags;
  const se_hip_mesh_view* views;   /* [n_views] */
} se_hip_mesh_select;
typedef struct se_hip_mesh_out {
  float* triangles;       /* [capacity_triangles][9] */
  int64_t capacity_triangles;
  int32_t* block_coords;  /* [capacity_blocks][3] */
  int64_t* block_range;   /* [capacity_blocks][2] */
  int64_t capacity_blocks;
  int64_t* header;        /* [4] */
} se_hip_mesh_out;
int se_hip_mesh_blocks(se_hip_pipeline* p, const se_hip_mesh_select* select, const se_hip_mesh_out* device_out);
int se_hip_mesh_blocks_host(se_hip_pipeline* p, const se_hip_mesh_select* select, const se_hip_mesh_out* host_out);

/* ---- batched axis-aligned region edits of the resident map: the reference's map write algorithm se::functor::axis_aligned_map(map, f, min, max)
 *      (se_core/include/se/functors/axis_aligned_functor.hpp) for N boxes at once, f = "assign x and / or y where the current value has one of
 *      these classes", without save / load.  The host restatement is include/se/axis_aligned.hpp (se::apply_edits is the executable definition).
 * An edit visits EXISTING blocks and nodes only and writes voxel / node VALUES only: nothing is allocated or freed, VoxelBlock::active_, the
 *   block and node counts and everything the raycast and the allocation scan derive from the set of blocks stay as they are.
 * A call applies the n edits as if one after another in list order (overlapping boxes: the later edit wins).
 *   lo, hi    the voxel box, half open [lo, hi) per axis -- the reference's (min, max).  An empty or inverted box is valid and selects no voxel
 *             (and no node value, except through the inclusive test of SE_HIP_EDIT_REFERENCE below when lo == hi).
 *   flags     SE_HIP_EDIT_SET_X: assign x; SE_HIP_EDIT_SET_Y: assign y (neither: nothing is written, the visits are still counted);
 *             SE_HIP_EDIT_BLOCKS: visit voxels; SE_HIP_EDIT_NODES: visit node values.
 *   only      the classes the CURRENT value may have for the edit to apply to it: bit 0 occupied, bit 1 unseen, bit 2 empty (1 << SE_HIP_COLLISION_*),
 *             7 = any.  The value (x, y), y as float as se_hip_download_blocks returns it, is classified with the call's `test` exactly as
 *             se_hip_collide_boxes classifies it.  `test` may be null when every edit has only == 7.
 *   Blocks    every voxel v of an allocated block with lo <= v < hi per axis (update_block).
 *   Nodes     SE_HIP_EDIT_REFERENCE  exactly update_node, quirks included (deliberate parity): the tested position starts at
 *                                    unpack_morton(code_) WITH the level bits still in the code and is advanced cumulatively by dir(i) * side / 2,
 *                                    i.e. with h = side / 2 the eight positions are c0 + (0,0,0), (h,0,0), (h,h,0), (2h,2h,0), (2h,2h,h),
 *                                    (3h,2h,2h), (3h,3h,3h), (4h,4h,4h); the box test is inclusive at both ends (lo <= v <= hi); value_[i] is
 *                                    written whether or not child i exists.
 *             SE_HIP_EDIT_STRICT     value_[i] is written iff the child octant [c + dir(i) * h, c + dir(i) * h + h)^3, c the node's corner,
 *                                    lies wholly inside [lo, hi).  Blocks are treated identically in both modes.
 * Invalid edits are skipped whole and counted, never applied in part, and read no map memory: a coordinate of lo or hi outside
 *   [-2^30, 2^30]; unknown flag bits; only outside 1 .. 7; only != 7 with a null test, a non-finite threshold or occupied_above other than
 *   0 / 1; a non-finite x with SET_X or y with SET_Y; for SDF a y (with SET_Y) that is not an integer in 0 .. 255 -- the device keeps the
 *   weight in a byte, the rule by which se_hip_load_map refuses a file.
 * counts (optional, int64[4], zeroed by the call): [0] (edit, voxel) applications that passed box and predicate, [1] the same for node
 *   values, [2] blocks with at least one application, [3] invalid edits.
 * Ordering: the call answers for, and modifies, the map after everything enqueued before it (a scan that ran on the side stream included; a
 *   later scan on the side stream waits for it).  An outstanding deferred raycast is launched FIRST: frame f's images show the map before the
 *   edit, as the eager schedule gives them.  The next sweep / raycast / query on the handle sees the edit.  The images and the image ring, the
 *   launch counters (SE_HIP_K_*) and the timing sums are left alone.  Row-sharded replicas and sharded-sweep handles each hold the whole map:
 *   the call edits the replica it is given, and keeping replicas equal is the caller's job (the same edits on every replica).
 * Both entries refuse n < 0, null edits with n > 0 and an unknown mode with SE_HIP_E_INVALID before any launch (n == 0 only zeroes counts),
 *   and report a sticky SE_HIP_E_CAPACITY like the other batched calls.
 *   se_hip_edit_boxes       device arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_edit_boxes_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
#define SE_HIP_EDIT_SET_X 1u
#define SE_HIP_EDIT_SET_Y 2u
#define SE_HIP_EDIT_BLOCKS 4u
#define SE_HIP_EDIT_NODES 8u
#define SE_HIP_EDIT_STRICT 0
#define SE_HIP_EDIT_REFERENCE 1
typedef struct se_hip_edit {
  int32_t lo[3], hi[3];   /* voxel box, half open [lo, hi) -- the reference's (min, max) */
  float x, y;             /* the values to assign */
  uint32_t flags;         /* SE_HIP_EDIT_SET_X | SET_Y | BLOCKS | NODES */
  uint32_t only;          /* classes the CURRENT value must have: bit 0 occupied, bit 1 unseen, bit 2 empty; 7 = any */
} se_hip_edit;            /* 40 bytes */
int se_hip_edit_boxes(se_hip_pipeline* p, const se_hip_edit* device_edits, int64_t n, const se_hip_collide_test* test,
                      int32_t mode, int64_t* device_counts);
int se_hip_edit_boxes_host(se_hip_pipeline* p, const se_hip_edit* host_edits, int64_t n, const se_hip_collide_test* test,
                           int32_t mode, int64_t* host_counts);

/* ---- batched region allocation of the resident map: the reference's Octree::allocate(key_t*, int) (se_core/include/se/octree.hpp:792-856; also
 *      reachable as Octree::insert, both exercised by multiscale_unittest.cpp) over the keys of every octant of a level that a list of voxel boxes
 *      touches, without fusing depth and without save / load.  It is what makes se_hip_edit_boxes usable on a fresh map or in a region the camera has
 *      not seen: allocate the region, then edit it.  The host restatement is include/se/allocate_region.hpp (se::allocate_boxes is the executable
 *      definition).
 *   lo, hi    the voxel box, half open [lo, hi) per axis.  An empty or inverted box is valid and requests nothing.
 *   level     0 = leaf level: the 8^3 voxel blocks; 1 .. leaf_level (log2(size) - 3) = the octants of that tree level (side size >> level), created as
 *             nodes without children below them (leaf_level names the blocks again).
 *   reserved  must be 0.
 * Box i requests every octant of its level whose cube intersects [lo, hi) clipped to the volume [0, size)^3.  After the call every requested octant
 *   and all its ancestors exist, and nothing else was created.  Created blocks hold initValue() in every voxel and have VoxelBlock::active_ = true,
 *   as allocate_level sets them (octree.hpp:841); created nodes hold initValue() in value_[8], as a node the allocation scan creates.  Octants that
 *   existed before, their values and their active flags are untouched.  The result does not depend on list order or on overlaps between boxes.
 * Relation to the reference: this equals Octree::allocate over the same key list EXCEPT for the keys[0] rule of unique_multiscale
 *   (algorithms/unique.hpp:64-79), which keeps the list's smallest key whatever its level and so walks it down along child 0 to a leaf when it is
 *   coarser than leaf level -- the quirk the OFusion allocation scan restates; this entry does not apply it.  Leaf-level lists (duplicates or not)
 *   give exactly the reference's blocks and nodes; coarse or mixed lists do once the list also holds the leaf block at (0, 0, 0); a purely coarse
 *   list differs by exactly that child-0 chain.
 * Invalid boxes are skipped whole and counted, and read no map memory: a coordinate of lo or hi outside [-2^30, 2^30]; level outside
 *   0 .. leaf_level; reserved != 0.
 * counts (optional, int64[4], zeroed by the call): [0] blocks created, [1] nodes created (ancestors included), [2] requested (box, octant) pairs
 *   after clipping -- the sum over the valid boxes of the cells of their clipped octant range, overlaps counted per box --, [3] invalid boxes.
 * new_keys (optional, capacity_words >= 1 words): the allocation scan's list format [count, key ...], keys in the reference's format (Morton code |
 *   level): one key per octant this call created BECAUSE IT WAS REQUESTED.  A requested octant that came into being within the call as the ancestor of
 *   a finer request is implied by that request's key and need not be listed; which of the two comes first is unspecified.  In any order: every key
 *   names a requested octant that did not exist before, none appears twice, and the ancestor closure of the keys together with the map before is the
 *   map after.  count is the number wanted; only capacity_words - 1 keys are written.  The list is fit to hand to se_hip_alloc_commit of a peer
 *   replica, whose block and node sets are then equal.  The order of the keys is unspecified.
 * Ordering, exactly as for se_hip_edit_boxes: an outstanding deferred raycast is launched FIRST (frame f's images show the map before the
 *   allocation); a scan on the side stream is joined; a later scan on the side stream waits for the call.  The next sweep / raycast / query on the
 *   handle sees the new octants, occupancy bits and beam-start marks included.  The launch counters (SE_HIP_K_*), the timing sums, the images and the
 *   image ring are left alone.
 * Capacity: a block or node pool that runs out raises the usual sticky SE_HIP_E_CAPACITY (the octants that did not fit are absent; reported by this
 *   call's host form and by the next stage call; acknowledged with se_hip_clear_overflow).  A dense grid cannot run out of blocks.
 * Row-sharded replicas and sharded-sweep handles each hold the whole map: the caller issues the same call on every replica, or hands new_keys to
 *   se_hip_alloc_commit of the peers.
 * Both entries refuse n < 0, null boxes with n > 0 and capacity_words < 1 with a non-null key list with SE_HIP_E_INVALID before any launch;
 *   n == 0 only zeroes the outputs (counts and the list's count word).
 *   se_hip_allocate_boxes       device arrays; enqueued on the handle's stream, asynchronous like the stage calls.
 *   se_hip_allocate_boxes_host  host arrays; staged through a device buffer the handle keeps (and grows); synchronises before it returns. */
typedef struct se_hip_alloc_box {
  int32_t lo[3], hi[3];   /* voxel box, half open [lo, hi) */
  int32_t level;          /* 0 = leaf level (8^3 blocks); 1 .. leaf_level = octants of that level (nodes without children below them) */
  uint32_t reserved;      /* must be 0 */
} se_hip_alloc_box;       /* 32 bytes */
int se_hip_allocate_boxes(se_hip_pipeline* p, const se_hip_alloc_box* device_boxes, int64_t n, int64_t* device_counts,
                          uint64_t* device_new_keys, int64_t capacity_words);
int se_hip_allocate_boxes_host(se_hip_pipeline* p, const se_hip_alloc_box* host_boxes, int64_t n, int64_t* host_counts,
                               uint64_t* host_new_keys, int64_t capacity_words);

/* ---- measurement (replaces TICK()/TOCK() + PerfStats, se_shared/timings.h:7-15) */
#define SE_HIP_K_ALLOC_SCAN 0
#define SE_HIP_K_ALLOC_COMMIT 1
#define SE_HIP_K_INTEGRATE 2 /* block sweep + node sweep, one launch */
#define SE_HIP_K_RAYCAST 3
#define SE_HIP_K_APPLY_BRICKS 4 /* sharded sweep: the other replicas' bricks written into this map */
#define SE_HIP_K_COUNT 5
/* HIP-event timing of every kernel launch on the handle's stream (off by default). */
int se_hip_enable_timing(se_hip_pipeline* p, int32_t on);
/* sum of launch durations [ms] and number of launches per kernel since the last reset */
int se_hip_get_timings(se_hip_pipeline* p, double ms_sum[SE_HIP_K_COUNT], int64_t launches[SE_HIP_K_COUNT], int32_t reset);
/* Kernel launches per kind since the last reset, counted on the host at enqueue time (no events, no synchronisation, does not flush a deferred
 * raycast): counts[SE_HIP_K_*], and counts[SE_HIP_K_COUNT] = launches that were the fused raycast + scan kernel (each of which also counts as one
 * raycast and one allocation scan).  Returns 1 if a deferred raycast is outstanding, else 0.  bench.py asserts with it that a timed region of K
 * frames holds K scans, K sweeps and K raycasts. */
int se_hip_get_launch_counts(se_hip_pipeline* p, int64_t counts[SE_HIP_K_COUNT + 1], int32_t reset);
/* Work counters behind the algorithmic-bytes figures of the roofline (instrumented kernel
 * variants, slower; off by default): out[0..7] = alloc probes, new keys, swept blocks, nodes,
 * get calls, interp calls, grad calls, ray hits -- accumulated since enabled / last read;
 * out[8..12] = raycast wave clocks (shader cycles): sum over waves of first-leaf search, march,
 * gradient+store, max wave lifetime, sum of LDS staging; out[13..15] reserved. */
int se_hip_enable_stats(se_hip_pipeline* p, int32_t on);
int se_hip_get_stats(se_hip_pipeline* p, uint64_t out[16], int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* SE_HIP_H */
