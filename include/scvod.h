/*
 * scvod.h -- C-ABI of the MI355X-native SCV-OD hot path (libscvod.so).
 *
 * This is the drop-in boundary for the hot path of Yixin-F/DR-Using-SCV-OD
 * (SURVEY.md section 8b).  The reference has no FFI of its own: the seam is plain
 * C++ member calls on `class SSC : public Utility` (include/ssc.h:7) and
 * `template<class PointT> class PatchWork` (include/patchwork.h:37-191).  Each
 * entry point below names the reference member it replaces (file:line into
 * /root/reference).  The C++ facade in dr-using-scv-od_amd/host/ keeps the
 * reference's class signatures and calls only the functions declared here.
 *
 * Conventions
 *   - every function returns int status: 0 = SCVOD_OK, <0 = error (no exceptions,
 *     no logging, no allocation visible to the caller except through the ctx);
 *     scvod_last_error(ctx) returns a human-readable message.
 *   - plain pointers and sizes only.  "h_" pointers are host memory owned by the
 *     caller, "d_" pointers are device (HBM) memory owned by the caller.
 *   - a ctx is single-owner and not thread-safe (the reference caller is
 *     single-threaded, src/main.cpp:9-12); one ctx per GPU / stream.
 *   - points are packed float4 {x, y, z, intensity} (pcl::PointXYZI without the
 *     padding, 16 B/point).
 *   - the library is GPU-only: if no gfx950 device / HIP runtime is usable,
 *     scvod_create fails with SCVOD_ERR_NO_DEVICE.  There is no CPU fallback.
 */
#ifndef SCVOD_H_
#define SCVOD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCVOD_OK 0
#define SCVOD_ERR_INVALID (-1)   /* bad argument / parameter combination           */
#define SCVOD_ERR_NO_DEVICE (-2) /* no usable HIP device (no CPU fallback exists)   */
#define SCVOD_ERR_HIP (-3)       /* HIP runtime error, see scvod_last_error         */
#define SCVOD_ERR_CAPACITY (-4)  /* batch larger than the ctx capacity              */
#define SCVOD_ERR_STATE (-5)     /* call order violated (e.g. fetch before run)     */

/* One scan holds at most 2^19 points (a 128-beam x 2048-column sweep is 262144): sort keys carry the point index in
 * 19 bits.  Larger scans are refused with SCVOD_ERR_CAPACITY. */
#define SCVOD_MAX_SCAN_POINTS 524288
/* A ctx holds at most 2^31 - 65 points in total (int32 scan offsets); in practice the ≈ 310 B/point arena of a 288 GB
 * device ends near 0.85 G points (scvod_arena_bytes). */

#define SCVOD_NUM_ZONES 4
#define SCVOD_MAX_PATCHES 1024 /* reference model has 504 (patchwork.h:48-49) */

/* per-point class written by Patchwork (patchwork.h:326-391) */
#define SCVOD_CLS_GROUND 0    /* emitted into cloud_out                         */
#define SCVOD_CLS_NONGROUND 1 /* emitted into cloud_nonground                   */
#define SCVOD_CLS_DROPPED 2   /* z < -1.8h, r outside (2.7, 80], patch size <= 10 */

/* ---- configuration --------------------------------------------------------------- */

/* The `ssc/` keys of config/<name>.yaml that the hot path reads (include/utility.h:283-313;
 * defaults are the nh.param<> defaults there).  Names drop the trailing underscore. */
typedef struct scvod_params {
    float sensor_height; /* 2.0  */
    float min_dis;       /* 0.0  */
    float max_dis;       /* 50.0 */
    float min_angle;     /* 0.0  */
    float max_angle;     /* 360  */
    float min_azimuth;   /* -30  */
    float max_azimuth;   /* 60   */
    float range_res;     /* 0.2  */
    float sector_res;    /* 1.2  */
    float azimuth_res;   /* 2.0  */
    float occupancy;     /* 0.6  */
    /* keys of the bounding-box refine / recognise step (ssc.cpp:437-467, 849-872), used only by
     * scvod_batch_cluster_types */
    float max_z;         /* 1.0  */
    float min_z;         /* -1.0 */
    float car_square;    /* 2.0  */
    int32_t toBeClass;   /* 1    */
    int32_t reserved;
} scvod_params;

/* Patchwork constants.  Hard-coded in the reference (patchwork.h:48-51, :115-129);
 * exposed here as a defaulted struct (scvod_pw_params_default). */
typedef struct scvod_pw_params {
    int32_t num_iter;                                /* 3  */
    int32_t num_lpr;                                 /* 20 */
    int32_t num_min_pts;                             /* 10 */
    int32_t num_rings_of_interest;                   /* 4 (= elevation_thr_.size(), patchwork.h:73) */
    int32_t num_sectors_each_zone[SCVOD_NUM_ZONES];  /* 16,32,54,32 */
    int32_t num_rings_each_zone[SCVOD_NUM_ZONES];    /* 2,4,4,4     */
    double th_seeds;                                 /* 0.3   */
    double th_dist;                                  /* 0.1   */
    double max_range;                                /* 80.0  */
    double min_range;                                /* 2.7   */
    double uprightness_thr;                          /* 0.707 */
    double adaptive_seed_selection_margin;           /* -1.1  */
    double elevation_thr[4];                         /* -1.2,-0.9984,-0.851,-0.605 */
    double flatness_thr[4];                          /* 0,0.000125,0.000185,0.000185 */
} scvod_pw_params;

void scvod_params_default(scvod_params* p);       /* utility.h:283-310 defaults */
void scvod_pw_params_default(scvod_pw_params* p); /* patchwork.h:48-51,115-129  */

/* Curved-voxel grid sizes exactly as SSC::SSC computes them (src/ssc.cpp:36-39):
 * (int)std::ceil((max - min) / res) in float. */
void scvod_grid_dims(const scvod_params* p, int32_t* range_num, int32_t* sector_num,
                     int32_t* azimuth_num, int32_t* bin_num);

/* ---- PODs -------------------------------------------------------------------------- */

/* struct PointAPRI, include/utility.h:96-106 (44 bytes, same field order) */
typedef struct scvod_apri {
    float x, y, z;
    float range;
    float angle;
    float azimuth;
    float intensity;
    int32_t range_idx;
    int32_t sector_idx;
    int32_t azimuth_idx;
    int32_t voxel_idx;
} scvod_apri;

/* Per-patch plane record written by the Patchwork kernel (state of normal_, pc_mean_,
 * singular_values_ after extract_piecewiseground, patchwork.h:339-343). */
typedef struct scvod_patch_plane {
    float normal[3];
    float mean[3];
    float sv[3];
    int32_t n_pts;      /* points binned into the patch (pc2czm)                   */
    int32_t n_ground;   /* |regionwise_ground_| after the last iteration            */
    int32_t status;     /* 0 skipped (size<=num_min_pts), 1 kept, 2 rejected: tilt,
                           3 rejected: elevation+flatness                           */
} scvod_patch_plane;

/* Result of one scan.  All pointers are host memory owned by the ctx, valid until the
 * next call that produces a scvod_scan_result on the same ctx. */
typedef struct scvod_scan_result {
    int32_t n_points;
    int32_t n_ground;     /* |cloud_out|        patchwork.h:362,377,381           */
    int32_t n_nonground;  /* |cloud_nonground|  patchwork.h:348-349,363,373-374   */
    int32_t n_dropped;
    int32_t n_apri;       /* |apri_vec| == |cloud_use|  ssc.cpp:174,193           */
    int32_t n_rejected;   /* pushes into cloud_eva_static, ssc.cpp:161-172        */
    int32_t n_voxels;     /* |hash_cloud|        ssc.cpp:253-280                  */
    int32_t n_patches;
    const uint8_t* cls;           /* [n_points] SCVOD_CLS_*                        */
    const int32_t* ground_idx;    /* [n_ground] input index of cloud_out[k]        */
    const int32_t* nonground_idx; /* [n_nonground] input index of cloud_nonground[k] */
    const scvod_patch_plane* planes; /* [n_patches] in (zone, ring, sector) order  */
    const scvod_apri* apri;       /* [n_apri] apri_vec                             */
    const int32_t* apri_src;      /* [n_apri] input index of apri_vec[k]/cloud_use[k] */
    const int32_t* rejected_src;  /* [n_rejected] input index, push order          */
    /* hash_cloud as CSR, voxels sorted by ascending voxel_idx key */
    const int32_t* vox_key;       /* [n_voxels] Voxel key (PointAPRI::voxel_idx)   */
    const int32_t* vox_pt_begin;  /* [n_voxels+1] offsets into vox_pts             */
    const int32_t* vox_pts;       /* [n_apri] Voxel::ptIdx, ascending per voxel    */
    const float* vox_av;          /* [n_voxels] Voxel::intensity_av  ssc.cpp:283   */
    const float* vox_cov;         /* [n_voxels] Voxel::intensity_cov ssc.cpp:284-287 */
} scvod_scan_result;

/* ---- context ------------------------------------------------------------------------- */

typedef struct scvod_ctx scvod_ctx;

/* max_points_total: capacity of the device arena in points summed over a batch;
 * max_scans: capacity in scans per batch.  pw may be NULL (defaults). */
int scvod_create(const scvod_params* params, const scvod_pw_params* pw, int device,
                 int64_t max_points_total, int32_t max_scans, scvod_ctx** out);
void scvod_destroy(scvod_ctx* ctx);
/* the parameters the ctx was created with */
int scvod_get_params(const scvod_ctx* ctx, scvod_params* out);
const char* scvod_last_error(const scvod_ctx* ctx);
/* bytes of HBM held by the ctx arena */
int64_t scvod_arena_bytes(const scvod_ctx* ctx);

/* ---- per-scan host entry points (what the SSC / PatchWork facade calls) ---------------- */

/* Replaces SSC::process up to and including makeHashCloud (src/ssc.cpp:224-241):
 * PatchWork::estimate_ground (patchwork.h:277-398) -> SSC::makeApriVec (ssc.cpp:155-195)
 * -> SSC::makeHashCloud (ssc.cpp:253-289).  h_xyzi: n x {x,y,z,intensity}. */
int scvod_process_scan(scvod_ctx* ctx, const float* h_xyzi, int32_t n, scvod_scan_result* out);

/* Replaces PatchWork::estimate_ground only (patchwork.h:105-109).  Fills the Patchwork
 * fields of `out`; the apri / voxel fields are zero. */
int scvod_patchwork(scvod_ctx* ctx, const float* h_xyzi, int32_t n, scvod_scan_result* out);

/* Replaces SSC::makeApriVec (ssc.cpp:155-195) on an arbitrary cloud (no Patchwork):
 * with apply_filter != 0 the range/FOV rejection of ssc.cpp:161-172 is applied,
 * with apply_filter == 0 every point is binned unclamped as in SSC::tracking
 * (ssc.cpp:1280-1286).  Followed by SSC::makeHashCloud when with_voxels != 0. */
int scvod_bin_scan(scvod_ctx* ctx, const float* h_xyzi, int32_t n, int32_t apply_filter,
                   int32_t with_voxels, scvod_scan_result* out);

/* Replaces SSC::makeHashCloud (ssc.cpp:253-289) on an apri_vec the caller already holds.  Fills the
 * voxel fields of `out` (and echoes the apri fields). */
int scvod_voxelize(scvod_ctx* ctx, const scvod_apri* h_apri, int32_t n, scvod_scan_result* out);

/* T = getTransformation(next)^-1 * getTransformation(pre), src/ssc.cpp:1255-1257
 * (pcl::getTransformation + Eigen::Affine3f inverse/product restated on the host).
 * pose = {x, y, z, roll, pitch, yaw}; T_out is row-major 3x4. */
void scvod_pose_delta(const float pose_pre[6], const float pose_next[6], float T_out[12]);

/* Bulk part of SSC::tracking (ssc.cpp:1274-1321): for every cluster c (points
 * h_xyzi[offsets[c] .. offsets[c+1]) ), transform by T (utility.h:394-406), re-bin
 * without range/FOV rejection (ssc.cpp:1280-1286), probe the next frame's voxel table
 * (sorted keys + labels) and keep hits whose label != -1 (ssc.cpp:1304-1305).
 *   h_hit_slot   [n_pts]        slot in the next table of the voxel hit by the point, or -1
 *   h_uniq_slots [n_pts]        per cluster: sorted unique hit slots (sampleVec, ssc.cpp:1319-1321)
 *   h_uniq_begin [n_clusters+1] offsets into h_uniq_slots
 * The label grouping / occupancy-ratio decisions (ssc.cpp:1323-1421) stay on the host
 * because they mutate the next frame sequentially. */
int scvod_track_probe(scvod_ctx* ctx, const float* h_xyzi, const int32_t* h_offsets,
                      int32_t n_clusters, const float T[12], const int32_t* h_next_keys,
                      const int32_t* h_next_labels, int32_t n_next_vox, int32_t* h_hit_slot,
                      int32_t* h_uniq_slots, int32_t* h_uniq_begin);

/* ---- loader step in front of the path ------------------------------------ */

/* SSC::getCloud's label filter + intensity scaling (src/ssc.cpp:1063-1076: points whose label & 0xFFFF is 0 or 1 are
 * skipped, intensity *= max_intensity) followed by pcl::VoxelGrid<pcl::PointXYZI>::filter with leaf (lx, ly, lz)
 * (src/ssc.cpp:1103-1106: 0.08 m; PCL 1.8.1 semantics incl. the "leaf size too small -> output = input" branch).
 * labels == NULL: VoxelGrid only (no filter, no scaling).  Output: one xyzi centroid per occupied cell in ascending
 * cell index, the cell's points summed in ascending input index (std::sort leaves that order unspecified in PCL).
 * d_* pointers are device memory; h_out_offsets[n_scans+1] receives the output offsets (in points).  The ctx's arena
 * is reused: results of an earlier scvod_batch_process are invalidated.  Synchronous. */
int scvod_batch_voxelgrid(scvod_ctx* ctx, const void* d_xyzi, const uint32_t* d_labels,
                          const int32_t* h_scan_offsets, int32_t n_scans, const float leaf[3],
                          float max_intensity, void* d_out_xyzi, int64_t out_capacity,
                          int32_t* h_out_offsets, void* stream);

/* The same for one scan in host memory. */
int scvod_voxelgrid(scvod_ctx* ctx, const float* h_xyzi, const uint32_t* h_labels, int32_t n,
                    const float leaf[3], float max_intensity, float* h_out_xyzi,
                    int32_t out_capacity, int32_t* n_out);

/* ---- device-resident batch entry points (sequence shards; used by bench.py) ------------- */

/* Run Patchwork -> binning -> voxel descriptors over n_scans scans already resident in
 * HBM.  d_xyzi: all scans concatenated; h_scan_offsets[n_scans+1] point offsets.
 * stream: hipStream_t (NULL = the ctx's own stream).  Asynchronous w.r.t. the host
 * unless sync != 0.  d_xyzi must stay valid and unchanged until the next batch call: apri_vec is kept
 * on the device in compact form (source index, voxel key, intensity) and the PointAPRI records,
 * the per-point class array and the tracking probe read the points through it on request.
 * h_scan_offsets is copied into the ctx before the call returns (also with sync == 0): the array is the caller's again at once, and
 * every later fetch reads the ctx's copy. */
int scvod_batch_process(scvod_ctx* ctx, const void* d_xyzi, const int32_t* h_scan_offsets,
                        int32_t n_scans, void* stream, int32_t sync);

/* Per-scan counters of the last batch: out[n_scans][8] =
 * {n_points, n_ground, n_nonground, n_dropped, n_apri, n_rejected, n_voxels, 0}.
 * Exactly the n_scans rows of the LAST batch are written, whatever the ctx's capacity: h_out behind them is left untouched, and
 * scvod_batch_fetch, scvod_batch_fetch_clusters, scvod_batch_fetch_cluster_types, scvod_batch_fetch_cluster_classes and
 * scvod_batch_fetch_track refuse a scan index >= that n_scans with SCVOD_ERR_INVALID -- the rows a larger, earlier batch left in the arena are never readable as live data. */
int scvod_batch_counts(scvod_ctx* ctx, int32_t* h_out);

/* Download the full result of scan `s` of the last batch.  vox_av / vox_cov: a batch's voxel stage leaves them out (nothing on the
 * device chain reads them unless the intensity merge is on); the first fetch of a batch computes them for all its scans with one
 * kernel on the batch's stream, later fetches find them there.  Same bits as the per-scan calls return
 * (scvod_set_voxel_descriptors chooses when they are computed, never what).  ground_idx / nonground_idx / rejected_src (and cls, built
 * from them): the emission of such a batch leaves the three lists out as well -- the first reader of a list (this call, the label /
 * class / export calls, a map accumulated without the ground or without the rejects) pays one pass over the batch, later readers
 * find them there; a ctx in scvod_set_voxel_descriptors mode 1 writes them in the emission, as the per-scan calls do. */
int scvod_batch_fetch(scvod_ctx* ctx, int32_t s, scvod_scan_result* out);

/* When the per-voxel intensity descriptors (vox_av / vox_cov) of a batch are computed.  mode 0 (the default): on demand -- at the
 * first scvod_batch_fetch of the batch, or before the intensity merge of a scvod_batch_cluster when scvod_set_intensity_merge was
 * turned on after the batch was processed; a ctx whose intensity merge is already on when the batch is processed computes them in
 * the voxel stage, since its clustering reads every one of them.  mode 1: eager, in the voxel stage of every batch.  The values are
 * bit-identical in both modes.  Takes effect with the next batch.  scvod_process_scan, scvod_bin_scan and scvod_voxelize return the
 * descriptors to the host at once and always compute them in the voxel stage.  SCVOD_ERR_INVALID for any other mode. */
int scvod_set_voxel_descriptors(scvod_ctx* ctx, int32_t mode);

/* Scan-vs-next-scan differencing of the whole batch on the device: SSC::tracking (src/ssc.cpp:1250-1426) for every scan
 * against its successor, the way SSC::segDF drives it (src/ssc.cpp:1449-1451).  Needs scvod_batch_cluster and
 * scvod_batch_cluster_types of the same batch: the clusters walked are those whose type is `car` (ssc.cpp:1262), the
 * successor's Voxel::label is the cluster of the voxel's points, -1 where refineClusterByBoundingBox erased it
 * (ssc.cpp:461-466), Cluster::occupy_voxels.size() the number of voxels carrying a label (ssc.cpp:382-392).
 *   h_T          [n_scans][12]  trans_next^-1 * trans_pre of (s, successor) (scvod_pose_delta); unused rows ignored
 *   h_next_scan  [n_scans] or NULL: successor of scan s -- an index of the batch, -1 = none (last scan of a sequence),
 *                -2 - e = the external table e.  NULL: s + 1, none for the last scan.
 *   h_ext_tables [n_ext] device pointers to tables written by scvod_batch_export_table on ANOTHER shard (the first scan of
 *                the next block of the sequence): how a block's last scan is tracked across a shard boundary.  A table may
 *                hold any number of voxels, 0 included (every car cluster tracked against it is then dynamic, and nothing
 *                behind its header is read); it need not fit the scans of THIS batch: one with more voxels than the batch's
 *                largest scan has points is decided all the same, by a slower path without the per-wave LDS bitset.
 * Per cluster: the transformed points are re-binned without range/FOV rejection (ssc.cpp:1280-1286) and looked up in the
 * successor's table; hits are grouped by label and de-duplicated (remap_name, ssc.cpp:1304-1321); Cluster::state follows
 * ssc.cpp:1323-1397, first against the successor in its freshly segmented state (all pairs in parallel), then -- mode
 * SCVOD_TRACK_CHAIN, the default -- with the re-labelling / cloud appending of ssc.cpp:1354-1372, 1378-1384, 1399-1419
 * replayed in sequence order on the device (scvod_set_track_mode below).  Per apri point a SCVOD_DYN_* byte.
 * No host synchronisation inside the call; h_T / h_next_scan / h_ext_tables are copied (and re-uploaded only when they
 * differ from the previous call). */
#define SCVOD_DYN_STATIC 0      /* member of a cluster that is not dynamic                                        */
#define SCVOD_DYN_DYNAMIC 1     /* member of a `car` cluster with state == 1                                      */
#define SCVOD_DYN_UNCLUSTERED 2 /* its cluster was erased by the bounding-box refine (listed static, ssc.cpp:450-454) */
int scvod_batch_track(scvod_ctx* ctx, const float* h_T, const int32_t* h_next_scan, const void* const* h_ext_tables,
                      int32_t n_ext, void* stream, int32_t sync);

/* What scvod_batch_track decides (default SCVOD_TRACK_CHAIN).
 *   SCVOD_TRACK_CHAIN        the reference's SEQUENTIAL chain (SSC::segDF, src/ssc.cpp:1449-1451): tracking(i, i + 1) appends
 *                            the transformed cloud of a static car cluster to its successor cluster (ssc.cpp:1378-1384),
 *                            splits hit voxels off a non-car cluster (ssc.cpp:1351-1372) or fuses the car clusters it
 *                            hits (ssc.cpp:1396-1419) BEFORE tracking(i + 1, i + 2) walks that frame.  Cluster states, the
 *                            per-point bytes and the dynamic counters of every scan with a successor in the batch are
 *                            those of that loop, cluster_set walked in ascending canonical name (created clusters after
 *                            the original ones, in creation order).  On the device the chain of each sequence is cut into
 *                            segments of `segment_steps` steps walked concurrently, each warmed up `warmup_steps` steps
 *                            earlier; a segment whose warm-up did not reproduce the state its predecessor really ended
 *                            in is walked again from that state, so the result never depends on the two lengths
 *                            (segment_steps 0 = the shortest segment whose walkers still fit the device one per CU (<= 256), the default;
 *                            warmup_steps -1 = keep; by default the warm-up is chosen per stream: 10 steps, two more for the next batch whenever more than a few segments had to be walked again, up to 16).  A scan tracked against an EXTERNAL table ends its
 *                            chain: across shard boundaries the decision is first-order -- keep a sequence on one shard.
 *   SCVOD_TRACK_FIRST_ORDER  every cluster against its successor's fresh segmentation (all pairs independent).
 * n_unique / pair_* of scvod_track_result always describe a cluster's OWN points against the fresh successor. */
#define SCVOD_TRACK_CHAIN 1
#define SCVOD_TRACK_FIRST_ORDER 0
#define SCVOD_TRACK_CHAIN_GENERIC 3 /* testing: the chain with every step through the kernel's generic (HBM-resident) step */
int scvod_set_track_mode(scvod_ctx* ctx, int32_t mode, int32_t segment_steps, int32_t warmup_steps);
/* Chain mode needs CHAINS: every scan is the successor of at most one scan of the batch and the table holds no cycle
 * (SCVOD_ERR_INVALID otherwise).  Many scans against one reference scan is a first-order question: SCVOD_TRACK_FIRST_ORDER.
 * The chain's workspace is a separate allocation made by the first scvod_batch_track that needs it (walkers x ~70 bytes x the pool
 * capacity: 16 GB for a seq-05 job, NOT part of scvod_arena_bytes); scvod_chain_workspace_bytes reports it. */
int64_t scvod_chain_workspace_bytes(scvod_ctx* ctx);
/* Points of appended clouds one segment's state can hold (0 = default: 8 x the largest scan of the batch).  The reference
 * appends a static car cluster's whole cloud to its successor at every step (ssc.cpp:1381), so a cloud grows for as long
 * as the object is tracked; a state that outgrows the capacity is reported (SCVOD_ERR_CAPACITY) by scvod_batch_fetch_track /
 * scvod_batch_track_stats, never truncated silently.  Workspace = segments x ~70 bytes x this number. */
int scvod_set_chain_capacity(scvod_ctx* ctx, int64_t pool_points);
/* ONE sequence over several shards (SSC::segDF's loop #1, ssc.cpp:1435-1445, is per scan; loop #2, :1449-1451, is a chain).
 * A shard processes a block of scans plus a HALO of earlier ones (warm-up steps x tracking stride) and one successor per chain
 * behind the block.  scvod_set_track_owned(first): scans below `first` are that halo -- walked over as a warm-up, never decided
 * (their per-point bytes stay those of the first-order pass and belong to the shard before).  After scvod_batch_track:
 *   scvod_batch_track_chains      h_first_scan[k] = first scan of chain k (which interleaved sub-sequence it is), returns the count
 *   scvod_chain_state_bytes       size of a boundary-state record of this job
 *   scvod_chain_export_state      which = 1: the state chain k ENDED in (a device buffer: send it to the shard that owns the next
 *                                 block); which = 0: the state the chain assumed at its first own step (its warm-up's snapshot).
 *                                 Record = int32 {entries, carried points, parts, valid}, entries, parts, carried points; valid = 1,
 *                                 0 (the chain has no such state) or 2 (the state needs more than cap_bytes: nothing but the header is written)
 *   scvod_batch_track_resume      h_d_states[k] = device pointer of the record the previous shard sent for chain k (NULL: none):
 *                                 compared with that snapshot (entries and parts bit for bit, the carried points per entry as a
 *                                 multiset: their order depends on where a walk started and nothing reads it); a chain whose warm-up did not reproduce it is walked
 *                                 again from the received state (and verified / walked on segment by segment, like inside one
 *                                 shard), then the per-point bytes are rebuilt.  scvod_batch_track_stats counts the checks and walks.
 *   scvod_batch_track_compare     the comparison alone: *h_differ = chains whose warm-up did NOT reproduce the received record
 *                                 (they would be walked again); nothing is changed.  Lets the shards of a job exchange their
 *                                 end states all at once and fall back to one-after-the-other only behind the first shard
 *                                 that reports a difference (pyshim/shard.py resolve_chain_boundaries).  Synchronises.
 * The result is the single-shard chain's, whatever the halo length.  A shard resumes at most once per scvod_batch_track. */
int scvod_set_track_owned(scvod_ctx* ctx, int32_t first_owned_scan);
/* the same per scan (a shard that holds blocks of several sequences): h_is_halo[s] != 0 marks scan s as halo; a chain's halo
 * scans must be its first ones */
int scvod_set_track_halo(scvod_ctx* ctx, const uint8_t* h_is_halo, int32_t n_scans);
int scvod_batch_track_chains(scvod_ctx* ctx, int32_t* h_first_scan, int32_t cap);
int64_t scvod_chain_state_bytes(scvod_ctx* ctx);
int scvod_chain_export_state(scvod_ctx* ctx, int32_t chain, int32_t which, void* d_dst, int64_t cap_bytes, void* stream);
int scvod_batch_track_resume(scvod_ctx* ctx, const void* const* h_d_states, int32_t n_states, void* stream, int32_t sync);
int scvod_batch_track_compare(scvod_ctx* ctx, const void* const* h_d_states, int32_t n_states, int32_t* h_differ, void* stream);
/* The comparison without a word read on the host: the chains whose warm-up did NOT reproduce the received record are ADDED to
 * *d_differ, a device word the caller cleared (and may all-reduce over RCCL afterwards); a record that did not fit the buffer
 * it was exported into (scvod_chain_export_state with a fixed-size exchange buffer: header word 3 = 2) counts as a difference.
 * Asynchronous on `stream`; nothing is changed.  h_d_states is copied before the call returns. */
int scvod_batch_track_compare_device(scvod_ctx* ctx, const void* const* h_d_states, int32_t n_states, int32_t* d_differ, void* stream);
/* h_out8 = {mode the last scvod_batch_track ran, segments (workgroups), segments verified against their predecessor's
 * end state, segments walked again after that check failed, error bits, segment_steps, warmup_steps, scans of the batch whose
 * Frame::max_name the clustering could not determine (scvod_batch_cluster_last_name status 1 / 2: the chain handed out a fresh
 * cluster number there where the reference re-uses the last one)}.  Synchronises.
 * Returns SCVOD_ERR_CAPACITY when a chain state did not fit the walkers' workspace (the result is then invalid). */
int scvod_batch_track_stats(scvod_ctx* ctx, int32_t* h_out8);

/* Tracking result of scan `s` of the last scvod_batch_track.  Pointers are host memory owned by the ctx, valid until the
 * next fetch.  Clusters are the `car` clusters of the scan in ascending canonical name (smallest apri index). */
typedef struct scvod_track_result {
    int32_t n_apri;
    int32_t n_clusters;
    int32_t n_car_points;
    int32_t n_dynamic_clusters;
    int32_t n_dynamic_points;
    int32_t reserved;
    const int32_t* cluster_root;  /* [n_clusters] canonical cluster name                                  */
    const int32_t* cluster_size;  /* [n_clusters] |occupy_pts|                                            */
    const int32_t* cluster_state; /* [n_clusters] Cluster::state: -1 untouched, 0 static, 1 dynamic       */
    const int32_t* n_unique;      /* [n_clusters] unique labelled voxels of the successor under the cluster */
    const int32_t* pair_begin;    /* [n_clusters+1] offsets into pair_label / pair_count                   */
    const int32_t* pair_label;    /* remap_name keys (canonical names in the successor), ascending         */
    const int32_t* pair_count;    /* remap_name[label].size() after sampleVec                              */
    const uint8_t* pt_dyn;        /* [n_apri] SCVOD_DYN_*                                                  */
} scvod_track_result;
int scvod_batch_fetch_track(scvod_ctx* ctx, int32_t s, scvod_track_result* out);

/* Publishes the successor tables of the batch: Voxel::label, cluster sizes and types of every scan (the table its
 * predecessor is tracked against; the clustering kernel writes them together with the clusters, this call checks that the
 * clustering and the box rules of the batch are current).  A sharded sequence calls this, exports the tables of its blocks'
 * first scans, exchanges them, and then calls scvod_batch_track.  Asynchronous on `stream`. */
int scvod_batch_track_tables(scvod_ctx* ctx, void* stream);

/* Boundary message of a sequence shard: writes 1 + n_voxels records of 16 bytes into d_out (device memory, capacity
 * cap_records): record 0 = {records that follow, n_voxels, 0, 0}, then per voxel of scan `s` in ascending key
 * {key, label, |occupy_voxels| of the label's cluster, its type (0 erased, 1 other, 2 car)}.  Asynchronous on `stream`.
 * The shard that owns the PREVIOUS scan of the sequence passes the buffer (after a device-to-device / RCCL transfer) as
 * an external table to scvod_batch_track. */
int scvod_batch_export_table(scvod_ctx* ctx, int32_t s, void* d_out, int64_t cap_records, void* stream);

/* Curved-voxel clustering of the last batch (SSC::clusterAndCreateFrame, src/ssc.cpp:299-352):
 * connected components of apri points under the reference's 3x3x3 occupied-voxel neighbourhood (grid
 * clipped, no sector wrap-around, findVoxelNeighbors ssc.cpp:395-411).  The partition equals the
 * reference's; cluster NAMES are canonical (smallest apri index of the cluster) instead of the
 * order-dependent 5, 6, 7... of the reference.  Results stay on the device until fetched. */
int scvod_batch_cluster(scvod_ctx* ctx, void* stream, int32_t sync);
/* The visiting order of clusterAndCreateFrame (ssc.cpp:322-340) only matters around index triples OUTSIDE the grid (a
 * return at polar angle exactly 0 has sector index -1, ...).  Scans whose tables fit the LDS (every 64-beam scan) are
 * clustered with the exact visiting-order model always.  Larger scans (128 beams on a fine grid) first ask a local rule
 * per irregular run -- do the cells around its triple and around its key's own cell settle that every find sticks? (the
 * statement: csrc/scvod_k_cluster.inc cc_run_is_plain, pinned against the reference loop by
 * tests/test_irregular_runs_rule.py) -- and model the visiting order exactly for the components of the runs it does not
 * settle (about one 128-beam scan in thirty has such a run): such a scan is handed to a second kernel (k_cc_exact) whose
 * workgroups cluster it again from scratch and SHARE the passes over an affected component -- the listed voxels of every node, the
 * Jacobi rounds of the labelling times, the joins -- with the blocks of that kernel that lead no scan (round 6).
 * on = 1 (the default since round 6): whatever the component's size (4-6 ms per 1000 128-beam scans; nothing for scans that fit the
 * LDS).  on = 0 (the default of rounds 3-5): while those components have <= 4096 nodes together; beyond that the scan keeps
 * "everything found is joined" for them (the reference's partition then refines the device's) and is counted.
 * on = 2: exact without the rule (every component with an irregular run is clustered again: what the rule is
 * tested against).  on = 3: like 1, every scan's workgroup on its own (the round-5 form of on = 1: tens of milliseconds for a
 * component of tens of thousands of nodes; A/B runs and the test of the shared passes).
 * scvod_batch_cluster_stats: h_out4 = {scans of the last clustering that kept the approximation, nodes
 * of the components concerned (upper bound), 1 when the bound is lifted (on = 1, 2, 3), scans beyond the LDS whose z-planes were
 * too large for the windowed search and were joined on a forest in HBM instead (slower, same result)};
 * scvod_batch_cluster_rule_stats: h_out2 = {irregular runs of those larger scans the rule settled, runs whose component
 * was clustered again}.  Both synchronise. */
int scvod_set_cluster_exact(scvod_ctx* ctx, int32_t on);
/* scvod_batch_cluster_help_stats: h_out2 = {workgroups of the last clustering that published their passes, chunks (1024 nodes of
 * one pass) that helper blocks took}.  Synchronises. */
int scvod_batch_cluster_help_stats(scvod_ctx* ctx, int32_t* h_out2);
int scvod_batch_cluster_stats(scvod_ctx* ctx, int32_t* h_out4);
int scvod_batch_cluster_rule_stats(scvod_ctx* ctx, int32_t* h_out2);
/* Frame::max_name.  clusterAndCreateFrame ends with `frame_ssc.max_name = cluster_name ++;` (ssc.cpp:354): the frame keeps
 * the LAST USED running number K, and the first cluster SSC::tracking splits off or fuses in that frame is called K again
 * (ssc.cpp:1357, :1401) -- when a cluster K is still alive the insert (:1372, :1419) is a no-op and the new cluster is lost.
 * scvod_batch_cluster therefore also determines, per scan, which cluster (canonical name) still carries K when the visiting
 * loop ends (csrc/scvod_lastname.hip), and the tracking chain hands that name out first.  literal = 0 switches both off:
 * every new cluster gets a fresh number (rounds 1-3 of this library).  Default 1.
 * scvod_batch_cluster_last_name: h_out4[s] = {canonical name of the cluster carrying K or -1 (K was merged away, or every cluster
 * that could carry it was erased by the bounding-box refine: such a cluster is no cluster any more and the pass does not walk it),
 * lowest voxel slot whose first point belongs to it or -1, status, events replayed}; status 0 = exact; 1 = the classes
 * that had to be replayed hold more than 32 767 voxels together (node numbers are 16-bit in the replay's lists; up to 8192 the
 * tables live in LDS, beyond that in arena scratch: the facades of a 128-beam scan) or do not fit the scan's scratch: reported as "none"
 * (the fourth word then holds the number of voxels the set has, when the triage pass already knew: 33-54 k on the 128-beam bench job); 2 = more than 256 points with
 * an index triple outside the grid: reported as "none".  h_stats4 (optional) = {scans with status 1, with status 2, 0, 0}. */
int scvod_set_max_name_literal(scvod_ctx* ctx, int32_t literal);
int scvod_batch_cluster_last_name(scvod_ctx* ctx, int32_t* h_out4, int32_t cap_scans, int32_t* h_stats4);
/* copies the cluster name of every apri point of scan s into h_pt_cluster[cap]; returns the count (>= 0)
 * or a negative status */
int scvod_batch_fetch_clusters(scvod_ctx* ctx, int32_t s, int32_t* h_pt_cluster, int32_t cap);
/* Bounding-box refine + the bounding-box part of recognize for the clusters of scvod_batch_cluster
 * (SSC::refineClusterByBoundingBox ssc.cpp:437-467, SSC::recognize ssc.cpp:849-872):
 * per apri point of scan s, h_type[i] = -1 when its cluster is erased (min z > 0, fewer than toBeClass
 * points, z extent < 0.2 m), `car_label` when bbox area <= car_square && min z < min_z && max z < max_z,
 * otherwise `other_label`: building and tree both (the reference separates them with PCL region growing;
 * scvod_batch_fetch_cluster_classes returns that split when scvod_set_region_growing turned the stage on).  The intensity merge (ssc.cpp:571-635) is applied only when scvod_set_intensity_merge turned it on: the types are
 * then those of the fused clusters.  Returns the count or a negative status. */
int scvod_batch_cluster_types(scvod_ctx* ctx, void* stream, int32_t sync);
int scvod_batch_fetch_cluster_types(scvod_ctx* ctx, int32_t s, int32_t car_label, int32_t other_label, int32_t* h_type,
                                    int32_t cap);
/* one-shot host version on an apri_vec the caller holds (voxelises it first; applies the ctx's intensity merge setting) */
int scvod_cluster(scvod_ctx* ctx, const scvod_apri* h_apri, int32_t n, int32_t* h_pt_cluster);
/* Intensity merge of the clusters, SSC::refineClusterByIntensity (ssc.cpp:571-635), run by scvod_batch_cluster when iterations
 * > 0.  The clustering kernel has evaluated the bounding-box rules already; the merge re-evaluates them (same rule) for the fused
 * clusters only, which gives what the reference's order -- merge, then box refine -- gives (ssc/iteration_, ssc/search_c_, ssc/intensity_diff_,
 * ssc/intensity_cov_).  Off by default (iterations = 0): nothing is launched and every output stays as it was.  With it on,
 * scvod_batch_fetch_clusters / scvod_batch_fetch_cluster_types / scvod_cluster return the fused partition (canonical names: the
 * smallest apri index of the fused cluster) and its types, and everything downstream reads it: the successor tables, the car lists,
 * the tracking chain, the per-point dynamic bytes, the static map; scvod_batch_cluster_last_name reports the fused cluster that
 * contains the carrier of max_name.  The visiting order of the stage is fixed as DESIGN.md section 2 states.
 * search_c must lie in 1..3: the neighbour walk looks up (2 search_c + 1)^2 grid rows per voxel, and the packed index triples
 * (clamped at -2 below the grid) reproduce findVoxelNeighbors up to that radius for every triple the range / FOV filter keeps.
 * The grid's range x azimuth row table and a bit per point of the largest scan share the LDS of one workgroup (160 KB): larger
 * grids are refused by scvod_batch_cluster.  A scan of n points whose neighbour pairs outgrow their scratch (4 n + 256 pairs before
 * de-duplication: 4 per point, and a slack per scan that lets small sparse scans through) keeps its partition and every reader
 * of the clustering (fetches, scvod_cluster, tracking, merge stats) then fails with SCVOD_ERR_CAPACITY.
 * SCVOD_ERR_INVALID for negative values or search_c outside 1..3.  Scratch of about 100 bytes per point of the ctx's capacity is allocated on the first merged
 * clustering (counted by scvod_arena_bytes). */
int scvod_set_intensity_merge(scvod_ctx* ctx, int32_t iterations, int32_t search_c, float intensity_diff, float intensity_cov);
/* h_out4 = {clusters before the merge, fusions recorded (all iterations), clusters after, scans with at least one fusion} of the
 * last clustering (zeros when the merge was off).  SCVOD_ERR_CAPACITY as above.  Synchronises. */
int scvod_batch_cluster_merge_stats(scvod_ctx* ctx, int32_t* h_out4);
/* Region growing of the large clusters, SSC::recognize / SSC::regionGrowing (ssc.cpp:797-860), run by scvod_batch_cluster_types on
 * its stream when `on`.  Candidates are the clusters that the box rule sends down its `square > car_square` branch.  Per candidate
 * (n points in apri index order): exact k nearest points (k_eff = min(k, n), the point itself included), PCA normal and curvature
 * (NormalEstimation), smooth-mode region growing (smoothness_deg, curvature_threshold, segments of min_segment .. 10^6 points kept),
 * building iff the kept points >= n * plane_fraction (in double), tree otherwise.  The reference's values are (1, 10, 20, 10, 1.2, 0.2).
 * Off by default: nothing is launched and every output stays as it was; with it on, no other output changes either.  The
 * conventions where PCL leaves the order open are fixed as DESIGN.md section 2 states.  SCVOD_ERR_INVALID for k outside 1..16,
 * min_segment < 1, an angle outside (0, 90] or a fraction outside [0, 1].  Chunk scratch (about 240 bytes per point of up to 2^23
 * points of scans) and outputs (21 bytes per point of the ctx's capacity) are allocated on first use (counted by scvod_arena_bytes). */
int scvod_set_region_growing(scvod_ctx* ctx, int32_t on, int32_t k, int32_t min_segment, double smoothness_deg,
                             float curvature_threshold, double plane_fraction);
/* per apri point of scan s: -1 erased, car_label, building_label or tree_label.  Without the stage (off, or not run on the last
 * clustering) every non-car cluster is tree_label.  Returns the count or a negative status. */
int scvod_batch_fetch_cluster_classes(scvod_ctx* ctx, int32_t s, int32_t car_label, int32_t building_label, int32_t tree_label,
                                      int32_t* h_type, int32_t cap);
/* the stage's per-point results for scan s: h_normal_curv (4 floats per apri point: normal, curvature; NaN for the points of
 * non-candidates) and h_segment (apri index of the seed that owns the point's segment, -1 for non-candidates); either may be NULL.
 * SCVOD_ERR_STATE unless the stage ran on the last clustering.  Returns the count or a negative status. */
int scvod_batch_fetch_region_growing(scvod_ctx* ctx, int32_t s, float* h_normal_curv, int32_t* h_segment, int32_t cap);
/* h_out8 = {candidate clusters, building clusters, candidate points, kept edges (p -> q, q != p), largest number of propagation
 * sweeps of a cluster, clusters on the HBM path (more than 8192 points), tail points, 0} of the last scvod_batch_cluster_types
 * (zeros when the stage did not run).  Synchronises. */
int scvod_batch_region_growing_stats(scvod_ctx* ctx, int32_t* h_out8);

/* Intensity calibration by incidence angle, SSC::intensityCalibrationByCurvature (ssc.cpp:98-153; the call at ssc.cpp:234-235), run
 * by every Patchwork run (scvod_batch_process, scvod_sequence_ingest, scvod_process_scan, scvod_patchwork) between the emission of
 * the non-ground cloud and the voxel stage when `on`.  Over the WHOLE non-ground cloud of a scan in emission order (the order of
 * nonground_idx; the points the range/FOV test rejects are neighbours too), per point: intensity clamped to max_intensity; the exact
 * k_eff = min(search_num, n) nearest points, itself included, by d^2 = (dx*dx + dy*dy) + dz*dz in fp32, ties by position; PCA
 * normal (NormalEstimation, NaN for fewer than 3 points); c = |n . p| / (|n| |p|), raised to (float)0.3 when below; the result
 * I0 / c capped at max_intensity.  A NaN normal gives NaN, as in the reference.  The calibrated value replaces PointAPRI::intensity
 * of the points that pass the range/FOV test (the apri records, hence vox_av / vox_cov, hence the intensity merge); nothing else
 * moves.  Limits: search_num 3..16; the static map keeps the RAW intensity of its points (it reads the input cloud);
 * scvod_bin_scan / scvod_voxelize on caller-supplied points are not calibrated.  Off by default: nothing is launched or allocated
 * and every output stays as it was.  SCVOD_ERR_INVALID (the setting stays as it was) for search_num outside 3..16 or a
 * max_intensity that is not a positive number -- also in a call that turns the stage off (on = 0): pass valid values there too.  Chunk scratch (36 bytes per point of up to 2^22 points of scans, plus 3 MB) is
 * allocated by the first calibrated batch (counted by scvod_arena_bytes).  Conventions: DESIGN.md section 2. */
int scvod_set_intensity_calibration(scvod_ctx* ctx, int32_t on, int32_t search_num, float max_intensity);
/* the stage's per-point results for scan s of the last batch, in nonground_idx order: h_normal_curv (4 floats per non-ground
 * point: normal, curvature) and h_intensity (the calibrated intensity); either may be NULL.  A batch keeps neither normals nor
 * neighbour lists: the call calibrates scan s again on the batch's stream (the input cloud must still be in place) and
 * synchronises.  SCVOD_ERR_STATE unless the stage ran on the last batch.  Returns n_nonground or a negative status. */
int scvod_batch_fetch_intensity_calibration(scvod_ctx* ctx, int32_t s, float* h_normal_curv, float* h_intensity, int32_t cap);
/* h_out8 = {non-ground points calibrated, intensities clamped before the division, cosines raised to 0.3, results capped at
 * max_intensity, NaN normals, queries that read candidates outside their workgroup's staged tile (the fallback path), largest
 * ring of cells a query probed, 0} of the last batch (zeros when the stage did not run).  Synchronises. */
int scvod_batch_intensity_calibration_stats(scvod_ctx* ctx, int32_t* h_out8);
/* candidates the kNN of the last batch examined, all queries together: a 64-bit count (1.3 x 10^11 per K64 batch), which is why it
 * is not the eighth word of the stats; read by tools/intensity_calibration_cost.py.  Synchronises. */
int scvod_batch_intensity_calibration_candidates(scvod_ctx* ctx, int64_t* h_out);

/* Streaming ingest of a sequence held in HOST memory (the reference reads one .bin per scan, SSC::getCloud
 * src/ssc.cpp:1040-1125): chunks of `chunk_scans` scans travel host -> device on a copy stream into one of two device
 * buffers while the previous chunk runs scvod_batch_process on the ctx's stream; after the launches of a chunk are
 * enqueued `fn(user, ctx, first_scan, n_scans, stream)` is called to enqueue the consumers of that chunk (clustering,
 * tracking, map accumulation) on `stream` -- the arena holds one chunk at a time; fn may be NULL.  h_xyzi should be
 * pinned; SCVOD_INGEST_REGISTER pins it for the duration of the call.  Synchronous: returns when every chunk is done. */
#define SCVOD_INGEST_REGISTER 1
typedef int (*scvod_chunk_fn)(void* user, scvod_ctx* ctx, int32_t first_scan, int32_t n_scans, void* stream);
int scvod_sequence_ingest(scvod_ctx* ctx, const float* h_xyzi, const int32_t* h_scan_offsets, int32_t n_scans,
                          int32_t chunk_scans, int32_t flags, scvod_chunk_fn fn, void* user);

/* hipEvent timing of the kernels of the last batch call, in launch order:
 * names[i] (static strings), ms[i].  Returns the number of entries (<= cap). */
int scvod_batch_timings(scvod_ctx* ctx, const char** names, float* ms, int32_t cap);
/* enable (1) / disable (0) per-kernel hipEvent timing for subsequent batch calls */
int scvod_set_timing(scvod_ctx* ctx, int32_t enabled);

/* ---- correspondence search (north_star "GICP correspondence search"; the reference's
 * real analogue is the kd-tree look-up of src/evaluate.cpp:79-145) ----------------------- */

/* Range of the three searches below: they are exact while every map and query coordinate lies within 25 000 cell edges of the grid
 * origin on each axis, |x - origin| <= 25000 * cell.  The cell edge is max(radius, 0.2f); scvod_nn_radius_search takes
 * radius / 0.98f once radius exceeds 0.198.  The origin is the map's min corner in the two host forms and 0 in the device form, so
 * a device-resident cloud searched with radius <= 0.2 may reach 5 km from the origin.  (The 27-cell probe allows the fp32 cell
 * coordinate 1 % of a cell; its three roundings use up to 0.45 % per point at that range -- DESIGN.md, A7.)  Beyond the bound a
 * neighbour may be missed.  Non-finite coordinates are unspecified: a NaN map point can poison a query's running best depending
 * on the order inside a bucket. */

/* For every query point: index of the nearest map point (ties: lowest index) and the
 * squared distance (fp32, ((dx*dx + dy*dy) + dz*dz)); h_within[q] = 1 if any map point
 * lies within `radius` (squared distance < radius^2: pcl radiusSearch non-empty, evaluate.cpp:95,104).  h_xyz arrays
 * are n x 3 floats.  Coordinates: finite, within 25 000 cell edges of the map's min corner (above). */
int scvod_nn_search(scvod_ctx* ctx, const float* h_map_xyz, int32_t n_map,
                    const float* h_query_xyz, int32_t n_query, float radius,
                    int32_t* h_nn_idx, float* h_nn_sqdist, uint8_t* h_within);

/* pcl::KdTreeFLANN::radiusSearch as src/evaluate.cpp:95,104 uses it (is anything inside the radius?): per query the
 * nearest map point with squared distance < radius^2 (FLANN keeps dist < r^2), or index -1 / distance +inf.  Unlike
 * scvod_nn_search it never looks beyond the radius, so queries far from the map cost one 27-cell probe: the cell edge is chosen so
 * that radius^2 <= (0.99 cell)^2, and every map point inside the radius is among the 27 cells.  Coordinates: finite, within
 * 25 000 cell edges of the map's min corner (above); the cell edge is max(radius, 0.2f), or radius / 0.98f above radius 0.198. */
int scvod_nn_radius_search(scvod_ctx* ctx, const float* h_map_xyz, int32_t n_map, const float* h_query_xyz,
                           int32_t n_query, float radius, int32_t* h_nn_idx, float* h_nn_sqdist);

/* The same search on arrays already resident in HBM (packed xyz, 12 B per point); asynchronous on `stream`
 * (NULL = the ctx's stream).  For sequence-scale evaluation without host round trips.  The grid origin is 0:
 * coordinates are finite and |x| <= 25000 * max(radius, 0.2f) on every axis (above), 5 km for radius <= 0.2. */
int scvod_nn_search_device(scvod_ctx* ctx, const float* d_map_xyz, int32_t n_map,
                           const float* d_query_xyz, int32_t n_query, float radius,
                           int32_t* d_nn_idx, float* d_nn_sqdist, uint8_t* d_within, void* stream);

/* ---- world-frame static map of a sequence, mergeable across shards -------------------------------------------------
 * Reference analogue: `*instance_map += *rgb_ptr` over the clusters that are not dynamic (SSC::saveSegCloud mode 3,
 * src/ssc.cpp:477-554) plus the ground clouds and range/FOV rejects of the evaluation block (ssc.cpp:1460-1480), each scan
 * moved to the world by pcl::getTransformation(pose) (ssc.cpp:1455-1458).  Kept as a set of occupied cells of edge `leaf`
 * with ONE representative point per cell chosen by an order-independent rule (smallest packed in-cell offset), so that
 * shards can accumulate independently and merge their record lists (the payload of the RCCL all_gather) into
 * bit-identical maps.
 * A point whose cell index leaves [-2^20, 2^20) on any axis, or has a NaN coordinate, is left out and counted: the next
 * scvod_map_export* call reports SCVOD_ERR_CAPACITY until scvod_map_clear.  The stored intensity is intensity * 256 clamped to
 * [0, 65535] and truncated; a NaN intensity is not specified (the cell is still recorded, its intensity bits are arbitrary).
 * scvod_map_points rounds in fp32: beyond about 2^17 cells from the origin the handed-out coordinate may sit on a face of its cell. */
typedef struct scvod_map scvod_map;
#define SCVOD_MAP_NO_GROUND 1       /* leave cloud_out (ground) out                                  */
#define SCVOD_MAP_NO_REJECTED 2     /* leave cloud_eva_static (range/FOV rejects) out                 */
#define SCVOD_MAP_IGNORE_DYNAMIC 4  /* raw map: keep the points scvod_batch_track marked dynamic too  */
/* The map in two parts, so that most of it is accumulated WHILE the batch is tracked (a second stream): tracking can only
 * remove members of `car` clusters (src/ssc.cpp:1262), everything else is final once scvod_batch_cluster_types ran.
 * The cell rule is order-independent, so part UNTRACKED + part TRACKED == one call without a part flag, bit for bit. */
#define SCVOD_MAP_PART_UNTRACKED 8  /* every kept point that is not a member of a car cluster (needs no tracking result) */
#define SCVOD_MAP_PART_TRACKED 16   /* the car-cluster members scvod_batch_track left static                            */
int scvod_map_create(int device, int64_t capacity_cells, float leaf, scvod_map** out);
/* Two kinds of map share the table, the hash, the probing and every export / merge / clear call; only the packing of a record's
 * 64-bit value differs.
 *   SCVOD_MAP_KIND_PLAIN     val = qx << 48 | qy << 32 | qz << 16 | qi16: the map described above (what scvod_map_create creates)
 *   SCVOD_MAP_KIND_LABELLED  val = qx << 48 | qy << 32 | qz << 16 | label << 8 | qi8: the RECOGNISED map -- `instance_map` in the colour
 *                            of each cluster's class (SSC::saveSegCloud mode 3, src/ssc.cpp:501-554, the ground clouds beside it,
 *                            ssc.cpp:1461-1486), the cloud src/plotObject.cpp reads back class by class.  qx, qy, qz are the plain
 *                            map's 16-bit offsets, label is the caller's byte (0..255), qi8 = (int)clamp(intensity, 0.f, 255.f):
 *                            truncated, not scaled (a NaN intensity is not specified, as above).  Insertion is the same single 64-bit
 *                            atomicMin, so a cell's representative is the point with the smallest (offset, label, intensity): a
 *                            measured point with ITS OWN label.  The rule is order-independent, and because the leading 48 bits are
 *                            the plain map's, the representative's xyz equals the plain map's for the same kept set, bit for bit.
 * One representative per cell is this library's design (the reference appends every point).
 * scvod_map_export, _export_parts, _export_parts_padded, _merge and _clear treat the value as opaque and work on both kinds; records
 * carry no mark of their kind, so merging the records of a map of the other kind CANNOT be detected -- keep the kinds apart.
 * scvod_map_create_kind: SCVOD_ERR_INVALID for an unknown kind (before a device is looked for). */
#define SCVOD_MAP_KIND_PLAIN 0
#define SCVOD_MAP_KIND_LABELLED 1
int scvod_map_create_kind(int device, int64_t capacity_cells, float leaf, int32_t kind, scvod_map** out);
/* the kind of the map (SCVOD_ERR_INVALID for NULL) */
int32_t scvod_map_kind(const scvod_map* map);
void scvod_map_destroy(scvod_map* map);
const char* scvod_map_last_error(const scvod_map* map);
int64_t scvod_map_capacity(const scvod_map* map);
int scvod_map_clear(scvod_map* map, void* stream);
/* pcl::getTransformation(x, y, z, roll, pitch, yaw) as a row-major 3x4 matrix */
void scvod_pose_matrix(const float pose[6], float T_out[12]);
/* adds the static points of every scan of ctx's last batch: h_poses [n_scans][6].  Asynchronous on `stream`; h_poses is turned
 * into matrices and copied before the call returns (poses that differ from the previous call's wait for `stream` first: the
 * map's one staging copy may still be in flight). */
int scvod_batch_map_accumulate(scvod_ctx* ctx, scvod_map* map, const float* h_poses, int32_t flags, void* stream);
/* the same for scans [first, first + count) of the batch only (a shard's own block, without its halo); h_poses still [n_scans][6].
 * Both refuse a labelled map with SCVOD_ERR_INVALID before anything is launched. */
int scvod_batch_map_accumulate_range(scvod_ctx* ctx, scvod_map* map, const float* h_poses, int32_t flags, int32_t first, int32_t count, void* stream);
/* occupied cells as 16-byte records {uint64 cell key, uint64 packed point} into device memory (NULL: count only);
 * *n_out = number of cells.  Synchronises `stream`.  Record order is unspecified (sort by key for a canonical order). */
int scvod_map_export(scvod_map* map, void* d_records, int64_t cap_records, int64_t* n_out, void* stream);
/* The same records grouped by OWNER for a reduce-scatter of the map over n_parts <= 64 shards (owner = a hash of the cell
 * key modulo n_parts, identical on every shard): h_counts[n_parts] receives the group sizes, group p starts at the sum of
 * the sizes before it.  Every shard sends group p to shard p (one all-to-all over xGMI: every link carries 1/n of the
 * map instead of everything converging on one root) and merges what it receives into the map of its own part.
 * Synchronises `stream`. */
int scvod_map_export_parts(scvod_map* map, int32_t n_parts, void* d_records, int64_t cap_records, int64_t* h_counts, void* stream);
/* The same grouping into FIXED-SIZE slots, without any host synchronisation (the form a timed multi-GPU step uses): group p
 * is written to d_records[p * cap_per_part .. (p + 1) * cap_per_part), the rest of a slot is padding (key ~0, skipped by
 * scvod_map_merge); d_counts (device, n_parts x int64, optional) receives the group sizes.  The all-to-all then moves
 * n_parts equal slots (all_to_all_single on device tensors).  A group that does not fit its slot is counted and reported
 * by the next scvod_map_export* call as SCVOD_ERR_CAPACITY.  Asynchronous on `stream`. */
int scvod_map_export_parts_padded(scvod_map* map, int32_t n_parts, void* d_records, int64_t cap_per_part, void* d_counts, void* stream);
/* inserts records exported by another shard (a record with key ~0 is padding and skipped).  Asynchronous. */
int scvod_map_merge(scvod_map* map, const void* d_records, int64_t n, void* stream);
/* the map as points: d_xyzi [cap][4] floats (cell origin + stored offset, intensity), optionally the records beside them.  On a
 * labelled map the intensity is the record's low 8 bits (an integer 0..255). */
int scvod_map_points(scvod_map* map, void* d_xyzi, void* d_records, int64_t cap, int64_t* n_out, void* stream);

/* ---- the recognised map: a label per cell (maps of kind SCVOD_MAP_KIND_LABELLED) ---------------------------------------------------
 * Adds a caller's own cloud, no batch context needed: the point at h_scan_offsets[s] + i of d_xyzi (packed float4, 16-byte aligned)
 * carries the byte d_labels[h_scan_offsets[s] + i], is moved by scvod_pose_matrix(h_poses + 6 s) with the expression of
 * scvod_batch_map_accumulate (T0*x + T1*y + T2*z + T3 per row, fp32, left to right, no contraction; h_poses NULL: the zero pose for
 * every scan, through the same expression) and is kept iff h_keep256[label] != 0 (h_keep256 NULL: every label is kept).
 * Stream-ordered; offsets, poses and the keep table are copied before the call returns, and the call never synchronises -- except
 * that offsets or poses which differ from the previous call's wait for `stream` first (the map's one staging copy of each may still
 * be in flight).  Refused with SCVOD_ERR_INVALID before anything is launched: a plain map, n_scans < 0, NULL offsets, offsets that
 * decrease or start below 0, NULL points or labels of a cloud that is not empty, a d_xyzi that is not 16-byte aligned.  A point whose
 * cell leaves the map's range, a NaN coordinate and a full table are counted and reported by the next scvod_map_export* call, as
 * for the plain map. */
int scvod_map_accumulate_labelled(scvod_map* map, const void* d_xyzi, const uint8_t* d_labels, const int32_t* h_scan_offsets, int32_t n_scans,
                                  const float* h_poses, const uint8_t* h_keep256, void* stream);
/* The recognised map of the ctx's last batch: every kept input point of scans [first, first + count) (count -1: to the end) under its
 * byte of scvod_batch_point_classes -- 1 ground, 2 rejected, 3 unclustered, 4 tree / other, 5 static car, 6 dynamic, 7 building (only
 * with the region growing on; without it no cell carries a 7).  The bytes of the whole batch are written into scratch of the map's own
 * (one byte per point, grow-only, scvod_map_scratch_bytes; scvod_arena_bytes does not move), then the kernel of
 * scvod_map_accumulate_labelled runs on the ctx's input cloud.  flags are the five SCVOD_MAP_* flags as a keep table over the byte:
 *   0 (SCVOD_PT_DROPPED) never; 1 unless SCVOD_MAP_NO_GROUND; 2 unless SCVOD_MAP_NO_REJECTED; 3, 4, 5, 7 always; 6 only with
 *   SCVOD_MAP_IGNORE_DYNAMIC -- the raw map, from which "everything but 6" is the static and "6" the dynamic cloud
 *   (scvod_map_points_labelled): unlike the plain raw map it needs the tracking result, which is what tells a 6 from a 5
 *   SCVOD_MAP_PART_UNTRACKED  keeps {1, 2, 3, 4, 7} (less the two NO_ flags) of bytes computed WITHOUT a tracking result
 *   SCVOD_MAP_PART_TRACKED    keeps {5}, and 6 with SCVOD_MAP_IGNORE_DYNAMIC, of bytes computed with one
 * The cell rule is order-independent: part UNTRACKED + part TRACKED == one call without a part flag, bit for bit.  With the same
 * flags the cells are those of scvod_batch_map_accumulate on a plain map, and so are the leading 48 bits of every value.
 * State rules and errors are those of scvod_batch_point_classes (flags SCVOD_MAP_IGNORE_DYNAMIC for part UNTRACKED, 0 otherwise):
 * SCVOD_ERR_STATE without a batch of scvod_batch_process, its clustering and its types, SCVOD_ERR_INVALID when the tracking result
 * is missing or stale.  SCVOD_ERR_INVALID also for a plain map, both part flags, an unknown flag bit, a scan range outside the batch
 * and a map on another device -- each before anything is launched.  Stream-ordered (stream NULL = the stream of the ctx's last
 * batch call); synchronises only as scvod_map_accumulate_labelled does for poses that changed, and when the scratch has to grow. */
int scvod_batch_map_accumulate_classes(scvod_ctx* ctx, scvod_map* map, const float* h_poses, int32_t flags, int32_t first, int32_t count,
                                       void* stream);
/* bytes of device scratch the batch form holds on this map (0 before its first call, and for NULL) */
int64_t scvod_map_scratch_bytes(const scvod_map* map);
/* scvod_map_points of a labelled map with the label byte of every cell beside it, restricted to the cells whose label is selected
 * (h_select256[label] != 0; NULL: all): d_xyzi [cap][4] floats, d_labels [cap] bytes, d_records [cap] 16-byte records, any of them
 * NULL; *n_out = the number of SELECTED cells.  SCVOD_ERR_CAPACITY when they outgrow cap (nothing is written at or behind cap);
 * SCVOD_ERR_INVALID for a plain map.  Synchronises `stream`.  Row i of the three outputs is the same cell; the order is unspecified. */
int scvod_map_points_labelled(scvod_map* map, void* d_xyzi, uint8_t* d_labels, void* d_records, int64_t cap, const uint8_t* h_select256,
                              int64_t* n_out, void* stream);

/* ---- asking the map: the cell of a point and the nearest representative around it (both kinds) ------------------------------------
 * Reads the table only: no record, no counter of the map, no scratch of the accumulate calls moves.  The point at h_scan_offsets[s] + i
 * of d_xyzi (packed float4, 16-byte aligned) is moved by the pose of scan s with the expression of the accumulate calls (products and
 * sums rounded one by one; h_poses NULL: the zero pose) and its OWN CELL is the key an accumulate would give it.  A key is present iff
 * it is met from its home slot before an empty slot and within 512 slots -- the bound insertion uses, so a key that any accumulate or
 * merge placed is always found and one whose insertion was dropped is absent.  With h_select256 (labelled maps only) a cell whose
 * label byte is not selected counts as empty for every output.
 * radius == 0 looks at the own cell only (d_nn_key and d_nn_sqdist must be NULL).  0 < radius <= 0.99f * leaf also looks at the 27
 * cells around the own cell (cells outside the +-2^20 range do not exist): a CANDIDATE is the representative of an occupied, selected
 * cell among them, decoded in fp32 as scvod_map_points does, ((float)c + (q + 0.5f) / 65536.0f) * leaf per axis, at squared distance
 * d = (dx*dx + dy*dy) + dz*dz in fp32 from the moved point, and it counts only when d < radius * radius.  The nearest wins, equal d
 * goes to the smaller key.  While fp32 rounding of the coordinates stays far below 0.01 * leaf (a few km from the origin at leaf 0.2)
 * this is the nearest representative of the whole map within the radius; the definition is the 27-cell one.
 * Every output is optional and holds one entry per input point at the input index h_scan_offsets[s] + i:
 *   d_result      one SCVOD_MAPQ_* byte.  It speaks about cells, the nn pair about distance: an occupied own cell whose representative
 *                 is farther than the radius is CELL with an empty nn pair.
 *   d_cell_val    the own cell's 64-bit value (what scvod_map_export hands out), ~0 when it is absent or the point has no cell
 *   d_nn_key, d_nn_sqdist   key and d of the nearest candidate, ~0 and +inf when there is none
 *   d_scan_counts [n_scans][4] is overwritten with the numbers of {CELL, NEAR, MISS, OUT} points per scan
 * When only d_result, d_cell_val or d_scan_counts are asked for, a point whose own cell is occupied never looks at its neighbours.
 * Stream-ordered against accumulate, merge and clear; offsets, poses and the select table are copied before the call returns, and the
 * call never synchronises with the host -- except as the accumulate calls do: offsets or poses that differ from the previous call's
 * wait for `stream` first (a query with the poses of the accumulate before it uploads nothing), and the first query allocates its
 * counters.  Using one map from two streams at once is the caller's business: nothing here orders them, and the staging copies and
 * the counters are one per map.
 * Refused with SCVOD_ERR_INVALID before anything is launched or written: a NULL map, a radius that is negative, NaN or above
 * 0.99f * leaf, an nn output with radius 0, a select table on a plain map, n_scans < 0, NULL offsets, offsets that decrease or start
 * below 0, NULL points of a cloud that is not empty, a d_xyzi that is not 16-byte aligned. */
#define SCVOD_MAPQ_MISS 0 /* own cell not occupied, and (radius > 0) no representative within the radius */
#define SCVOD_MAPQ_CELL 1 /* own cell occupied                                                            */
#define SCVOD_MAPQ_NEAR 2 /* own cell not occupied, a representative of the 27 cells is within the radius */
#define SCVOD_MAPQ_OUT 3  /* the point has no cell: its coordinates are NaN or beyond +-2^20 cells         */
int scvod_map_query(scvod_map* map, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses, float radius,
                    const uint8_t* h_select256, uint8_t* d_result, uint64_t* d_cell_val, uint64_t* d_nn_key, float* d_nn_sqdist,
                    int64_t* d_scan_counts, void* stream);
/* The same for the input cloud of the ctx's last batch, every input point included (those Patchwork dropped too); h_poses
 * [n_scans][6].  SCVOD_ERR_STATE without a processed batch of input clouds, SCVOD_ERR_INVALID for a map on another device, both before
 * anything is launched; stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_map_query(scvod_ctx* ctx, scvod_map* map, const float* h_poses, float radius, const uint8_t* h_select256, uint8_t* d_result,
                          uint64_t* d_cell_val, uint64_t* d_nn_key, float* d_nn_sqdist, int64_t* d_scan_counts, void* stream);
/* h_out8 = {points, CELL, NEAR, MISS, OUT, 0, 0, 0} of the last query.  Synchronises that query's stream.  SCVOD_ERR_STATE before the
 * first query. */
int scvod_map_query_stats(scvod_map* map, int64_t* h_out8);
/* bytes of device memory the queries hold on this map: their counters (0 before the first query, and for NULL).
 * scvod_map_scratch_bytes and scvod_arena_bytes do not move. */
int64_t scvod_map_query_scratch_bytes(const scvod_map* map);

/* ---- cleaning scans against a prior map: every scan split into its known, novel and cell-less points ------------------------------
 * Reference analogue: none (the reference keeps its map as a PCL cloud and has no such program); sides and vote rule are this
 * library's convention.
 * Cloud, offsets, poses, radius, select table, the point's transform and its OWN CELL are exactly those of scvod_map_query, the staging
 * and stream-order rules included: offsets, poses, parameters and the select table are copied before the call returns, a filter with
 * the poses of the accumulate or query before it uploads nothing, and the call synchronises with the host only as scvod_map_query does
 * (offsets or poses that changed; a scratch that has to grow).  params NULL = the defaults.
 * OWN SIDE.  d_result (optional) is the byte scvod_map_query writes for the same arguments, before any vote.  A point's own side is
 * SCVOD_MAPF_KNOWN for CELL or NEAR, SCVOD_MAPF_NOVEL for MISS, SCVOD_MAPF_OUT for OUT.  With a radius, a point whose own cell is
 * occupied never looks at its neighbours; no nn pair is produced here.
 * VOTE (SCVOD_MAPF_OBJECT_VOTE, scvod_batch_map_filter only).  For every object of the table that the last scvod_batch_objects left
 * in the ctx's scratch (the state rules of scvod_batch_object_truth; a SCVOD_OBJ_NO_TRACK table is fine) the results of its member
 * points are counted.  An object with n_points >= min_points VOTES: it is KNOWN iff
 *     (int64)(n_cell + n_near) * vote_den >= (int64)vote_num * n_points
 * and NOVEL otherwise -- integers only, so host and device agree by construction.  A member whose own result is not OUT takes its
 * object's verdict as its side.  OUT members and every point that is no member of a voting object (ground, rejected, dropped and
 * unclustered points, members of objects below min_points) keep their own side.  d_votes (optional) receives one
 * scvod_map_filter_object per object in table order; nothing is written at or behind cap_votes, an overflow is latched for
 * scvod_map_filter_stats and changes no side and no other output.
 * OUTPUTS, each optional, each exactly as many entries as the input (no capacity, no overflow):
 *   d_side         one SCVOD_MAPF_* byte per input point at the input index
 *   d_order        the stable three-way partition PER SCAN: with b = h_scan_offsets[s], d_order[b + j] lists the in-scan indices of the
 *                  KNOWN points ascending, then the NOVEL ones ascending, then the OUT ones ascending
 *   d_bounds       int32 [n_scans][2] on the device: {n_known, n_known + n_novel} of scan s
 *   d_xyzi_out     d_xyzi_out[b + j] = the input record d_xyzi[b + d_order[b + j]] bit for bit (sensor frame; the intensity word and NaN
 *                  payloads travel); 16-byte aligned
 *   d_payload_out  the same gather of d_payload_in (one uint32 per input point); refused without d_payload_in
 * The partition works on tiles of SCVOD_MAP_FILTER_TILE consecutive points of one scan; no workgroup waits for another.
 * The call reads the table only: no record and no counter of the map moves, scvod_map_query_stats keeps describing the last QUERY, and
 * scvod_map_query_scratch_bytes, scvod_map_scratch_bytes, scvod_arena_bytes, the object table's and the truth stage's scratch do not
 * move.  The filter's scratch is one grow-only allocation of its own, owned by the map and freed with it, sized from the points and
 * scans of the largest call.  Stream-ordered against accumulate, merge, clear and query.
 * Refused with SCVOD_ERR_INVALID before anything is launched, written or allocated: everything scvod_map_query refuses; reserved != 0;
 * an unknown flag bit; vote_den < 1, vote_num < 0, vote_num > vote_den, vote_den > 1 << 20; min_points < 1; the vote flag on
 * scvod_map_filter; d_votes without the flag, or cap_votes < 0; an output that overlaps the input cloud; a d_xyzi_out that is not
 * 16-byte aligned (d_order, d_bounds, the payloads: 4-byte; d_votes: 4-byte); d_payload_out without d_payload_in.  scvod_batch_map_filter:
 * SCVOD_ERR_STATE as scvod_batch_map_query (no processed batch) and, with the vote, as scvod_batch_object_truth (no usable table). */
#define SCVOD_MAPF_KNOWN 0 /* the map knows the point (own cell occupied, or a representative within the radius) or its object */
#define SCVOD_MAPF_NOVEL 1
#define SCVOD_MAPF_OUT 2   /* SCVOD_MAPQ_OUT: the point has no cell; a vote never moves a point into or out of this side */
#define SCVOD_MAPF_OBJECT_VOTE 1 /* flags bit 0, batch form only */
#define SCVOD_MAP_FILTER_TILE 2048 /* points per tile of the partition */
typedef struct scvod_map_filter_params { /* 24 bytes */
    float radius;               /* as scvod_map_query: 0 = own cell only, at most 0.99f * leaf */
    int32_t flags;
    int32_t vote_num, vote_den; /* an object is KNOWN iff (int64)(n_cell + n_near) * vote_den >= (int64)vote_num * n_points */
    int32_t min_points;         /* objects with fewer members do not vote: their points keep their own side */
    int32_t reserved;           /* 0 */
} scvod_map_filter_params;
/* radius 0, flags 0, vote 1 / 2, min_points 1, reserved 0 */
void scvod_map_filter_params_default(scvod_map_filter_params* p);
typedef struct scvod_map_filter_object { /* 32 bytes, one per object of the table, table order */
    int32_t n_cell, n_near, n_miss, n_out; /* the members' SCVOD_MAPQ_* results */
    int32_t n_points;                      /* == scvod_object::n_points */
    int32_t verdict;                       /* SCVOD_MAPF_KNOWN / SCVOD_MAPF_NOVEL; -1: below min_points, did not vote */
    int32_t reserved[2];                   /* 0 */
} scvod_map_filter_object;
int scvod_map_filter(scvod_map* map, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                     const scvod_map_filter_params* params, const uint8_t* h_select256, uint8_t* d_result, uint8_t* d_side, int32_t* d_order,
                     int32_t* d_bounds, void* d_xyzi_out, const uint32_t* d_payload_in, uint32_t* d_payload_out, void* stream);
/* The same for every input point of the ctx's last batch, as scvod_batch_map_query; h_poses [n_scans][6]; stream NULL = the stream of
 * the ctx's last batch call.  d_votes: [cap_votes] scvod_map_filter_object records or NULL. */
int scvod_batch_map_filter(scvod_ctx* ctx, scvod_map* map, const float* h_poses, const scvod_map_filter_params* params,
                           const uint8_t* h_select256, uint8_t* d_result, uint8_t* d_side, int32_t* d_order, int32_t* d_bounds, void* d_xyzi_out,
                           const uint32_t* d_payload_in, uint32_t* d_payload_out, void* d_votes, int64_t cap_votes, void* stream);
/* h_out8 = {points, KNOWN, NOVEL, OUT, points the vote moved NOVEL->KNOWN, points it moved KNOWN->NOVEL, objects that voted, objects
 * that voted and came out KNOWN} of the last filter (without the vote flag the last four are 0).  Synchronises that filter's stream.
 * SCVOD_ERR_CAPACITY after a d_votes overflow, with h_out8 filled; SCVOD_ERR_STATE before the first filter. */
int scvod_map_filter_stats(scvod_map* map, int64_t* h_out8);
/* bytes of device memory the filter holds on this map (0 before the first call, and for NULL) */
int64_t scvod_map_filter_scratch_bytes(const scvod_map* map);

/* ---- the result of a batch handed on: per-point labels and the cleaned scans, on the device -------------------------------
 * Reference analogue: the `static_pt` / `dynamic_pt` lists of SSC::saveSegCloud mode 3 (src/ssc.cpp:477-554) and the clouds of the
 * evaluation block (`cloud_eva_static`, `g_cloud_vec`, the _static / _dynamic / _original .pcd files, ssc.cpp:1454-1540).  The
 * static map above keeps one point per cell; these two calls hand out the scans themselves.  Both are stream-ordered (stream NULL =
 * the stream of the ctx's last batch call), launch and allocate nothing unless they are called, never synchronise with the host,
 * change no other output of the batch, and read marks of their own: what the static map reads per input point stays as it was.
 *
 * One byte per INPUT point, index scan_offsets[s] + i: */
#define SCVOD_PT_DROPPED 0       /* in neither Patchwork cloud: SCVOD_CLS_DROPPED (outside the range gate, below the z cut, a
                                    patch of at most num_min_pts points)                                                     */
#define SCVOD_PT_GROUND 1        /* member of cloud_out                                                                       */
#define SCVOD_PT_REJECTED 2      /* non-ground, failed the range/FOV test (cloud_eva_static, rejected_src)                    */
#define SCVOD_PT_UNCLUSTERED 3   /* apri point whose cluster refineClusterByBoundingBox erased (SCVOD_DYN_UNCLUSTERED)        */
#define SCVOD_PT_STATIC_OTHER 4  /* apri point of a cluster that is neither dynamic nor `car`                                 */
#define SCVOD_PT_STATIC_CAR 5    /* apri point of a `car` cluster that is not dynamic (state -1, a scan without a successor,
                                    included)                                                                                 */
#define SCVOD_PT_DYNAMIC 6       /* pt_dyn == SCVOD_DYN_DYNAMIC                                                               */
#define SCVOD_PT_STATIC_BUILDING 7 /* scvod_batch_point_classes only: a SCVOD_PT_STATIC_OTHER point whose cluster the region growing
                                      classed as building                                                                     */
/* Writes the labels of the last batch into d_labels (device memory of `cap` >= the batch's point count bytes; SCVOD_ERR_CAPACITY
 * otherwise).  The type is the segmentation's, what scvod_batch_fetch_cluster_types reports (the fused partition's when the
 * intensity merge is on), not the type the tracking chain re-assigns to a predecessor at ssc.cpp:1354; the region growing's
 * building / tree split is not carried into the byte (scvod_batch_point_classes carries it).  Needs scvod_batch_cluster and scvod_batch_cluster_types of the batch
 * (SCVOD_ERR_STATE) and a CURRENT scvod_batch_track -- the validity test scvod_batch_map_accumulate applies; SCVOD_ERR_INVALID when
 * the tracking result is missing or stale.  flags: 0 or SCVOD_MAP_IGNORE_DYNAMIC -- the clustering and the types suffice then,
 * and no point is labelled SCVOD_PT_DYNAMIC. */
int scvod_batch_point_labels(scvod_ctx* ctx, uint8_t* d_labels, int64_t cap, int32_t flags, void* stream);
/* scvod_batch_point_labels with the region growing's building / tree split carried into the byte: the same contract (state rules,
 * errors, flags, stream order, no host synchronisation), the same bytes, except that an apri point which would be SCVOD_PT_STATIC_OTHER
 * gets SCVOD_PT_STATIC_BUILDING when the class of its cluster is building -- what scvod_batch_fetch_cluster_classes reports for it once
 * the region growing ran on the last scvod_batch_cluster_types.  Without the region growing every non-car cluster is tree and no point
 * gets 7: the output is scvod_batch_point_labels' byte for byte.  scvod_batch_point_labels itself, the export and the static map never
 * see the value 7. */
int scvod_batch_point_classes(scvod_ctx* ctx, uint8_t* d_classes, int64_t cap, int32_t flags, void* stream);
/* The kept points of every scan of the last batch, compacted: scans concatenated in batch order, inside a scan in INPUT order (a
 * stable compaction: the output is bit-identical from run to run).  The keep rule is that of scvod_batch_map_accumulate and a
 * function of the label byte alone: SCVOD_PT_DROPPED never; SCVOD_PT_DYNAMIC only with SCVOD_MAP_IGNORE_DYNAMIC; SCVOD_PT_GROUND
 * unless SCVOD_MAP_NO_GROUND; SCVOD_PT_REJECTED unless SCVOD_MAP_NO_REJECTED; everything else always.  The part flags (and any
 * other bit) are refused with SCVOD_ERR_INVALID; the state the call needs is that of scvod_batch_point_labels with the same flags.
 *   d_xyzi_out     [cap_points] packed float4 records, or NULL: count only (the offsets and the sizes are still produced, nothing
 *                  else is written)
 *   d_out_offsets  [n_scans + 1] device array: scan s owns the records [d_out_offsets[s], d_out_offsets[s + 1]); always the TRUE sizes
 *   d_src_out      [cap_points] or NULL: the input index inside its scan of every exported point
 *   d_payload_in   [batch points] or NULL: one uint32 per input point (e.g. SemanticKITTI labels), carried along into
 *   d_payload_out  [cap_points] or NULL
 *   h_poses        NULL: sensor frame, the records are the input's bit for bit.  Otherwise [n_scans][6] poses, turned into matrices
 *                  as scvod_batch_map_accumulate does (scvod_pose_matrix) and staged before the call returns -- the array is the
 *                  caller's again at once; a point moves by T0*x + T1*y + T2*z + T3 per row, evaluated left to right in fp32 without
 *                  contraction (the map kernel's expression); the intensity is untouched.
 * When the kept points outgrow cap_points nothing is written at or behind the capacity, and the overflow is latched until the next
 * export.  Scratch (one byte per point and 12 floats per scan of the ctx's capacity, one word per 2048 points of a scan) is
 * allocated by the first export and is NOT part of scvod_arena_bytes. */
int scvod_batch_export_points(scvod_ctx* ctx, int32_t flags, const float* h_poses, const uint32_t* d_payload_in, void* d_xyzi_out,
                              uint32_t* d_payload_out, int32_t* d_src_out, int64_t cap_points, int32_t* d_out_offsets, void* stream);
/* h_out4 = {points written, points kept (the capacity the export needs), 1 when the last export outgrew its buffers, 0} of the last
 * scvod_batch_export_points (points written is 0 for a count-only call).  Synchronises that export's stream.  Returns
 * SCVOD_ERR_CAPACITY when the last export overflowed, SCVOD_ERR_STATE before the first export. */
int scvod_batch_export_stats(scvod_ctx* ctx, int64_t* h_out4);

/* ---- the clusters of a batch as an object table, on the device ---------------------------------------------------------------
 * Reference analogue: Frame::cluster_set as SSC::segDF leaves it per scan -- Cluster::name / type / state / bounding_box / occupy_pts /
 * occupy_voxels (include/utility.h:142-162; src/ssc.cpp:377-385, 437-467, 844-872) and the box columns of the feature row that
 * getDescriptorByEigenValue fills (ssc.cpp:723-751).  Listed are exactly the members of cluster_set after
 * refineClusterByBoundingBox: the clusters whose type is not "erased".  Order: scans in batch order, inside a scan ascending canonical
 * name; the table is bit-identical from run to run.  One record is 64 bytes: */
typedef struct scvod_object {
    int32_t scan;        /* index of the scan in the batch                                                                      */
    int32_t name;        /* canonical cluster name: the smallest apri index of the cluster, scan-local (the fused cluster's name
                            with the intensity merge on)                                                                        */
    int32_t n_points;    /* occupy_pts.size()                                                                                   */
    int32_t n_voxels;    /* occupy_voxels.size() after sampleVec: the distinct voxel_idx among the cluster's points
                            (ssc.cpp:365, 383) -- also where a voxel's first point belongs to another cluster                   */
    float box_min[3];    /* pcl::getMinMax3D over the cluster's points (ssc.cpp:421-425): plain float min / max, exact and       */
    float box_max[3];    /*   order-independent (-0 orders below +0)                                                             */
    float center[3];     /* getCenterOfCloud (ssc.cpp:427-435): three sequential fp32 sums over the cluster's points in ascending
                            apri index, each divided by (float)n_points, no contraction                    */
    float angle_diff;    /* f_11(0, 8) = fabs(getPolarAngle(point_max) - getPolarAngle(point_min)) (ssc.cpp:731-733), with
                            PointAPRI::angle's float expression                                                                  */
    int8_t cls;          /* 1 tree / other, 2 car, 3 building (only when the region growing ran on the last
                            scvod_batch_cluster_types): what scvod_batch_fetch_cluster_classes reports                           */
    int8_t state;        /* Cluster::state of a car cluster as scvod_batch_fetch_track's cluster_state reports it; -1 for every
                            other cluster, and everywhere with SCVOD_OBJ_NO_TRACK                                                */
    uint8_t dynamic;     /* 1 iff the cluster's points carry SCVOD_DYN_DYNAMIC                                                   */
    uint8_t reserved;    /* 0                                                                                                    */
    int32_t point_begin; /* first slot of the cluster's members in the member list, counted over the whole batch                */
} scvod_object;
/* The remaining columns of the reference's 11-value feature row follow from the record and are not stored: point_max.z = box_max[2];
 * square = (double)(box_max[0] - box_min[0]) * (double)(box_max[1] - box_min[1]) (the library's cc_box_square); point_min.z =
 * box_min[2]; the six constants 1.0 (or the six values scvod_batch_object_shapes computes); type = cls: scvod_feature_row.
 *
 * scvod_batch_objects is stream-ordered (stream NULL = the stream of the ctx's last batch call), never synchronises with the host,
 * launches and allocates nothing unless it is called, reads the arena and writes only the caller's buffers and scratch of its own
 * (allocated on first use, NOT part of scvod_arena_bytes: scvod_batch_objects_scratch_bytes reports it; about 28 bytes per point of
 * the ctx's capacity plus the sort's workspace once a call asks for more than the counts).  Needs scvod_batch_cluster and
 * scvod_batch_cluster_types of the batch (SCVOD_ERR_STATE) and a CURRENT scvod_batch_track (SCVOD_ERR_INVALID when it is missing or
 * stale), exactly as scvod_batch_point_labels; with SCVOD_OBJ_NO_TRACK the clustering and the types suffice.  Any other flag bit is
 * SCVOD_ERR_INVALID.
 *   d_objects        [cap_objects] scvod_object records, or NULL: no records
 *   d_obj_offsets    [n_scans + 1] device array: scan s owns the records [d_obj_offsets[s], d_obj_offsets[s + 1]); always the TRUE sizes
 *   d_member_src     [cap_members] or NULL: per object, in table order, the INPUT index inside its scan (apri_src) of every member
 *                    point in ascending apri index -- occupy_pts in the form scvod_batch_export_points' d_src_out and a caller's own
 *                    per-point payload can be joined with.  point_begin is filled whether or not the list is asked for
 *   d_point_object   [batch points] or NULL: per INPUT point the index of its object in the table, -1 for the points of no object
 * Nothing is written at or behind cap_objects / cap_members; the offsets and the stats still report the true sizes; the overflow is
 * latched until the next call. */
#define SCVOD_OBJ_NO_TRACK 1 /* clustering + types suffice; state -1, dynamic 0 everywhere */
int scvod_batch_objects(scvod_ctx* ctx, int32_t flags, void* d_objects, int64_t cap_objects, int32_t* d_obj_offsets,
                        int32_t* d_member_src, int64_t cap_members, int32_t* d_point_object, void* stream);
/* h_out4 = {objects written, objects found, member slots needed, 1 when the last call outgrew a buffer} of the last
 * scvod_batch_objects.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow, SCVOD_ERR_STATE before the first call. */
int scvod_batch_objects_stats(scvod_ctx* ctx, int64_t* h_out4);
/* bytes of device scratch the object table holds on this ctx (0 before the first call) */
int64_t scvod_batch_objects_scratch_bytes(scvod_ctx* ctx);

/* ---- the eigenvalue descriptor of the table's objects, on the device (opt-in: nothing runs unless it is called) -------------------
 * Reference analogue: the part of SSC::getDescriptorByEigenValue that the reference holds as text and leaves switched off
 * (src/ssc.cpp:659-721, constants include/utility.h:246-253, 318-325, YAML keys feature/k*_), and SSC::compareFeature
 * (ssc.cpp:897-911).  Per object of the table, from its member points in ascending apri index:
 *   centroid     pcl::compute3DCentroid: the rule of scvod_object::center, recomputed (the caller's table is not read)
 *   cov          pcl::computeCovarianceMatrix(cloud, centroid, cov) of PCL 1.8, NOT normalised: six sequential fp32 chains
 *   eig          the singular values of that symmetric matrix by Eigen's JacobiSVD (the Patchwork specification), ascending.  The
 *                reference asks Eigen::EigenSolver; this convention is parity-unpinned
 *   feat         in double, literally as written at ssc.cpp:680-718 with e_i = eig[i] / (double)(eig[0] + eig[1] + eig[2]); log and pow
 *                are fdlibm's log / exp restated (scvod_math.h), the same bits on the host and on the device
 * Divisions by zero and 0 * -inf stay what IEEE makes of them; such objects are flagged and counted, not repaired.  96 bytes: */
typedef struct scvod_object_shape {
    float cov[6];    /* xx, xy, xz, yy, yz, zz                                                                                   */
    float eig[3];    /* ascending: eig[0] is the smallest                                                                        */
    int32_t flags;   /* bit 0: some feature is not finite; bit 1: n_points < 3                                                   */
    double feat[7];  /* linearity, planarity, scattering, omnivariance, anisotropy, eigen_entropy, change_of_curvature          */
} scvod_object_shape;
typedef struct scvod_feature_params {
    double kOneThird, kLinearityMax, kPlanarityMax, kScatteringMax, kOmnivarianceMax, kAnisotropyMax, kEigenEntropyMax,
        kChangeOfCurvatureMax;
} scvod_feature_params;
/* the nh.param<> defaults of utility.h:318-325: 0.333, 740, 959, 1248, 0.278636, 1248, 0.956129, 0.99702 */
void scvod_feature_params_default(scvod_feature_params* p);
/* the constants the next shape calls of this ctx use (a new ctx holds the defaults).  Checked before any device is looked for:
 * SCVOD_ERR_INVALID for a NULL argument, a kOneThird that is not finite and a k*Max that is not a positive finite number. */
int scvod_set_object_features(scvod_ctx* ctx, const scvod_feature_params* p);
/* One scvod_object_shape per object of the LAST scvod_batch_objects call of this batch that asked for records, members or the
 * per-point objects (it left the sorted member list in the table's scratch), in table order, into d_shapes [cap_shapes].
 * Stream-ordered (stream NULL = the stream of the ctx's last batch call; the table call must be ordered before it), never
 * synchronises, reads the arena and the table's scratch and writes d_shapes and four stats words of its own (allocated by the first
 * call and counted by scvod_batch_objects_scratch_bytes: + 32 bytes; scvod_arena_bytes does not change).  SCVOD_ERR_STATE when no such
 * table call was made (a count-only call is none) or when the clustering changed since; otherwise the state the table call needed is
 * needed again, with its flags: SCVOD_ERR_STATE without clustering and types of the batch, SCVOD_ERR_INVALID when the table read a
 * tracking result that is stale now.  Nothing is written at or behind cap_shapes; the overflow is latched until the next call. */
int scvod_batch_object_shapes(scvod_ctx* ctx, void* d_shapes, int64_t cap_shapes, void* stream);
/* h_out4 = {records written, objects of the table, written records with flags bit 0, 1 when the table outgrew cap_shapes} of the
 * last scvod_batch_object_shapes.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow, SCVOD_ERR_STATE before
 * the first call. */
int scvod_batch_object_shapes_stats(scvod_ctx* ctx, int64_t* h_out4);
/* Host only, no device.  The 11-value row of ssc.cpp:686-751: columns 0-5 = feat[0..5] (the six constants 1.0 when shape is NULL:
 * the row the reference builds today), 6 = box_max[2], 7 = cc_box_square, 8 = angle_diff, 9 = box_min[2], 10 = cls. */
void scvod_feature_row(const scvod_object* object, const scvod_object_shape* shape, double* out11);
/* Host only.  SSC::compareFeature literally: float diff = 0; diff += |a[i] - b[i]| * w[i] with the double weights 0.5, 0.5, 0.2,
 * 0.2, 0.2, 0.2, 0.2, 0.6, 0.2, 0.0 of ssc.cpp:900-909 (column 10 is not read). */
float scvod_compare_feature(const double* a, const double* b);

/* ---- the ESF descriptor of an object, on the device (opt-in: nothing runs or is allocated unless it is called) ----------------------
 * Reference analogue: SSC::getDescriptorByEnsembleShape (src/ssc.cpp:760-786: pcl::ESFEstimation's 640-bin signature folded to ten
 * values) and SSC::getFeature21 (ssc.cpp:788-795: the 11-value row and those ten).  Parity is unpinned by construction: PCL seeds
 * rand() with time(0), so the reference's numbers do not repeat, and ssc.cpp:773 folds into an uninitialised array.  The convention
 * here keeps the structure of PCL 1.8's features/impl/esf.hpp with a counter-based sampler (the esf_* functions
 * of csrc/scvod_math.h are the definition).  All fp32, in the written order, no contraction:
 *   extent     c = the centroid by the sequential sums of scvod_object::center; q = p - c; r = sqrt(max(qx*qx + qy*qy + qz*qz));
 *              u = q * (32.0f / r).  r zero or not finite: flags bit 2
 *   voxels     of a coordinate v: v < 0 ? floor(v) + 32 : ceil(v) + 31, clamped to 0..63; every point sets the 3x3x3 voxels around
 *              its own in a 64^3 occupancy grid
 *   sampler    sample k draws i_j = mulhi32(mix(seed + 0x9E3779B9 * (3k + j + 1)), n), j = 0, 1, 2, with mix the 32-bit finaliser
 *              h ^= h>>16; h *= 0x7feb352d; h ^= h>>15; h *= 0x846ca68b; h ^= h>>16: a function of (seed, k, n) alone, so an object's
 *              descriptor does not depend on the batch around it.  An invalid sample is skipped, never redrawn
 *   valid      the indices differ pairwise and, with a, b, c the distances 12, 13, 23 and s = (a+b+c)*0.5f,
 *              ((s*(s-a))*(s-b))*(s-c) > 0.001f
 *   lines      12, 13, 23 between the voxels A, B of the two points: with d = B - A and m = max |d_i|, t = 0..m visits
 *              A_i + sgn(d_i) * ((2|d_i| t + m) / (2m)) (integers); count = m + 1, in = the visited voxels that are set.  IN iff
 *              in >= count - 1, else OUT iff in <= 7, else MIX with ratio (float)in / (float)count
 *   triangle   OUT iff sum(in) <= 21, else IN iff sum(count) - sum(in) < 4, else MIX
 *   bins       ten histograms of 64 integer counters: A3 in/out/mix (three corner bins per sample, by triangle class; the bin of
 *              x = min(1, |dot| / (len1*len2)) is the number of b in 1..63 with x <= (float)cos((b - 0.5) pi / 126)), D3 in/out/mix
 *              (sqrt(sqrt(heron)) / max_d3), D2 in/out/mix (a, b, c by their own line's class, / max_d2), ratio (MIX lines); a
 *              value v in [0, 1] falls into bin (int)floor(v * 63.0f + 0.5f); the maxima are those of the object's valid samples
 *   signature  sig[h*64 + b] = value * w[h], value = (float)count / 3.0f for the A3 rows, else (float)count,
 *              w = {.5, .5, .5, .5, .5, 1, 1, 2, 2, 2}; total = the sequential sum over i = 0..639; sig[i] /= total
 *   fold10     fold10[j] = (float) of the double sum of sig[i] over ascending i with i % 10 == j
 * Every number is the same bits on the device, in the CPU helper of the tests and from run to run.  64 bytes: */
typedef struct scvod_object_esf {
    float fold10[10];   /* the ten values getDescriptorByEnsembleShape returns                                                    */
    int32_t n_valid;    /* samples that passed the validity tests                                                                */
    int32_t n_points;
    int32_t flags;      /* bit 0: no valid sample; bit 1: fewer than min_points points; bit 2: zero or non-finite extent; bit 3:
                           left out by cls_mask.  A flagged record has fold10 and its signature all zero, never NaN              */
    uint32_t lines[3];  /* lines of the valid samples that were IN / OUT / MIX                                                    */
} scvod_object_esf;
typedef struct scvod_esf_params {
    int32_t samples;     /* point triples drawn per object, 1 .. 65536 (PCL: 20000)                                              */
    uint32_t seed;
    int32_t min_points;  /* objects of fewer points are flagged, not computed; at least 3                                        */
    uint32_t cls_mask;   /* bit c selects the objects with cls == c; read by scvod_batch_object_esf only                         */
    int32_t reserved[4]; /* 0                                                                                                    */
} scvod_esf_params;
/* 20000, 0, 3, 0xFFFFFFFF */
void scvod_esf_params_default(scvod_esf_params* p);
/* One record per object of a cloud the caller groups: d_xyzi holds 16-byte xyzi records on the device, d_begin [n_objects + 1] int32
 * on the device; object o is the run [d_begin[o], d_begin[o + 1]) in the given order (an empty run is an object of no points).
 * params NULL = the defaults.  d_records [cap] scvod_object_esf; d_sig640 NULL or float [cap][640], the normalised signatures.
 * Stream-ordered (stream NULL = the ctx's stream), never synchronises; reads the inputs and writes the two buffers and scratch of
 * its own (scvod_esf_scratch_bytes; scvod_arena_bytes and every other stage's scratch stay as they are).  Argument errors
 * (SCVOD_ERR_INVALID: a NULL ctx, d_records, or d_xyzi / d_begin with n_objects > 0; n_objects or cap negative; samples outside
 * 1..65536; min_points < 3; misaligned pointers) are reported before a device is looked for.  Nothing is written at or behind cap;
 * the overflow is latched until the next call.  The ESF calls of a ctx share its counters and scratch: a call on another stream
 * than the ctx's last ESF call waits for that call on the device (an event, no host synchronisation), so they never overlap. */
int scvod_esf_device(scvod_ctx* ctx, const float* d_xyzi, const int32_t* d_begin, int64_t n_objects, const scvod_esf_params* params,
                     void* d_records, float* d_sig640, int64_t cap, void* stream);
/* The same on the table the last scvod_batch_objects left in its scratch: the members of an object in ascending apri index, gathered
 * as scvod_batch_object_shapes gathers them; cls_mask selects by scvod_object::cls (the others get flags bit 3).  State rules and
 * error codes are exactly those of scvod_batch_object_shapes (stream NULL = the stream of the ctx's last batch call); a
 * SCVOD_OBJ_NO_TRACK table is fine.  One rule more, because the mask reads the class bytes: SCVOD_ERR_STATE when
 * scvod_batch_cluster_types ran since that table call (its records may show other classes): call scvod_batch_objects again. */
int scvod_batch_object_esf(scvod_ctx* ctx, const scvod_esf_params* params, void* d_records, float* d_sig640, int64_t cap, void* stream);
/* h_out8 = {records written, objects, written records with flags != 0, 1 when the objects outgrew cap, valid samples summed over
 * the written records, objects left out by cls_mask, objects whose points did not fit the on-chip cache (SCVOD_ESF_CACHE_POINTS),
 * 0} of the last ESF call.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow, SCVOD_ERR_STATE before the
 * first call. */
int scvod_esf_stats(scvod_ctx* ctx, int64_t* h_out8);
#define SCVOD_ESF_CACHE_POINTS 3584 /* objects of up to this many points are sampled from on-chip memory */
/* bytes of device scratch the ESF stage holds on this ctx (0 before the first call) */
int64_t scvod_esf_scratch_bytes(scvod_ctx* ctx);
/* Host only.  fold10 of a normalised 640-value signature, as the record holds it. */
void scvod_esf_fold10(const float* sig640, float* out10);
/* Host only.  SSC::getFeature21: columns 0-10 are scvod_feature_row(object, shape), columns 11-20 esf->fold10 as doubles. */
void scvod_feature_row21(const scvod_object* object, const scvod_object_shape* shape, const scvod_object_esf* esf, double* out21);

/* ---- evaluation against labelled truth, on the device (opt-in: nothing runs or is allocated unless it is called) ------------------
 * Reference analogue: tool/analysis.py:124-194 -- the counters behind the published PR / RR / F1 table -- and the colour classes of the
 * map viewer (src/evaluate.cpp:79-145).  A ground-truth point is an INLIER when its nearest estimate point (squared distance
 * d = (dx*dx + dy*dy) + dz*dz in fp32, ties to the lowest estimate index) satisfies sqrt((double)d) < voxelsize * sqrt(3.0) / 2, evaluated
 * in double exactly as written.  A label is DYNAMIC when (label & 0xFFFF) is in the class list.  The look-up is one 27-cell probe of a hash
 * grid with cell edge max(voxelsize, 0.2): the inlier radius is 0.87 cell edges, so the nearest candidate inside it is the true nearest
 * neighbour and a point without one has no inlier -- there is no second pass.  All counts are integer sums: the same on every run. */
typedef struct scvod_eval_params {
    double voxelsize;            /* analysis.py's voxelsize: positive and finite                                         */
    int32_t n_dynamic_classes;   /* 0..16                                                                                */
    uint16_t dynamic_classes[16];
} scvod_eval_params;
/* voxelsize 0.2, the classes 252..259 (analysis.py:6, config ssc/dynamic_label_) */
void scvod_eval_params_default(scvod_eval_params* p);
typedef struct scvod_eval_result {
    int64_t num_gt_static, num_gt_dynamic, num_est_static, num_est_dynamic, num_preserved, num_static_preserved, num_dynamic_preserved;
    double PR, RR, F1;
} scvod_eval_result;
/* Host only, no device.  counts: the seven counts in the order of the struct.  PR = 100.0 * num_static_preserved / num_gt_static,
 * RR = 100.0 * (num_gt_dynamic - num_dynamic_preserved) / num_gt_dynamic, F1 = 2 * (PR / 100) * (RR / 100) / ((PR / 100) + (RR / 100))
 * when PR + RR > 0, else 0.0: the double operations of analysis.py:186-190 in their order.  A rate whose denominator is 0 is NaN, and
 * F1 is then NaN: analysis.py would raise there; reporting NaN is this library's choice. */
void scvod_eval_finish(const int64_t counts[7], scvod_eval_result* out);
/* Ground truth (d_gt_xyz packed at 12 B per point as in scvod_nn_search_device, d_gt_label uint32) against an estimate cloud of the same
 * form.  d_point_result: NULL, or one byte per gt point: bit 0 inlier, bit 1 gt dynamic, bit 2 estimate dynamic at the neighbour (set only
 * together with bit 0: a point without an inlier has no neighbour); nothing per point is written without it.  Stream-ordered (stream
 * NULL = the ctx's stream), never synchronises with the host; each call overwrites the counters of the one before, and the evaluation
 * calls of one ctx must be ordered among themselves (they share the scratch).  Argument errors (NULL ctx, negative sizes, a NULL array of
 * a non-empty cloud, more than 16 classes, a voxelsize that is not positive and finite) are SCVOD_ERR_INVALID before any device is
 * looked for.  Scratch (the grid and the counter words; for the batch form also world xyz, a keep byte and a label byte per point and
 * 12 floats per scan) is an allocation of its own, grow-only, freed by scvod_destroy and NOT part of scvod_arena_bytes; a call that
 * needs more than any before waits for the evaluation in flight before it grows. */
int scvod_evaluate_device(scvod_ctx* ctx, const float* d_gt_xyz, const uint32_t* d_gt_label, int32_t n_gt, const float* d_est_xyz,
                          const uint32_t* d_est_label, int32_t n_est, const scvod_eval_params* params, uint8_t* d_point_result,
                          void* stream);
/* The ERASOR protocol for the ctx's last batch: ground truth is EVERY input point of the batch in the world frame (h_poses [n_scans][6],
 * the expression of scvod_batch_export_points, staged before the call returns) with its label d_gt_label [batch points]; the estimate is
 * the points scvod_batch_export_points would keep with the same `flags`, carrying the same labels -- as a keep mask over the same world
 * array: the export is stable, so the tie rule sees the export's order.  State rules and errors are those of scvod_batch_point_labels
 * with the same flags (SCVOD_MAP_NO_GROUND, SCVOD_MAP_NO_REJECTED, SCVOD_MAP_IGNORE_DYNAMIC; the part flags are refused).  No output
 * of the batch changes.  The whole batch is evaluated: a shard that wants to leave its halo out exports its own scans and calls
 * scvod_evaluate_device itself.  Stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_evaluate(scvod_ctx* ctx, const uint32_t* d_gt_label, const float* h_poses, int32_t flags, const scvod_eval_params* params,
                         uint8_t* d_point_result, void* stream);
/* counts and rates (scvod_eval_finish) of the last scvod_evaluate_device / scvod_batch_evaluate.  Synchronises that call's stream.
 * SCVOD_ERR_STATE before the first evaluation. */
int scvod_evaluate_stats(scvod_ctx* ctx, scvod_eval_result* out);
/* bytes of device scratch the evaluation holds on this ctx (0 before the first call) */
int64_t scvod_evaluate_scratch_bytes(scvod_ctx* ctx);
/* evaluate() of src/evaluate.cpp:79-145 per point of the original map (d_orig_xyz packed xyz, d_pred_static one byte per point, != 0:
 * predicted static): s15 / s10 = a point of the static cloud lies at squared distance < r15*r15 / r10*r10 (products in fp32), d15 / d10
 * the same for the dynamic cloud; then, in this order, predicted static and s15 -> 1 (TP_STATIC), predicted static, not s15, d10 -> 2
 * (FN_STATIC), predicted dynamic and d15 -> 3 (TN_DYNAMIC), predicted dynamic, not d15, s10 -> 4 (FN_DYNAMIC), otherwise 0 (UNMATCHED).
 * An empty cloud matches nothing.  d_class: one byte per point, or NULL (counts only).  The grids' cell edge is 0.2, so r15 and r10
 * must be positive and at most 0.198 (evaluate.cpp's are 0.15 and 0.10); SCVOD_ERR_INVALID otherwise.  Stream rules, scratch and argument
 * errors as scvod_evaluate_device; the class counters are words of their own (an evaluation in between leaves them alone). */
int scvod_classify_map_device(scvod_ctx* ctx, const float* d_orig_xyz, const uint8_t* d_pred_static, int32_t n, const float* d_static_xyz,
                              int32_t n_static, const float* d_dynamic_xyz, int32_t n_dynamic, float r15, float r10, uint8_t* d_class,
                              void* stream);
/* h_out5 = points of class 0 .. 4 of the last scvod_classify_map_device.  Synchronises that call's stream.  SCVOD_ERR_STATE before the
 * first call. */
int scvod_classify_map_stats(scvod_ctx* ctx, int64_t* h_out5);

/* ---- a map split by the nearest-neighbour hits of a cleaned cloud, on the device (opt-in: nothing runs or is allocated unless it is
 * called) ---------------------------------------------------------------------------------------------------------------------------
 * Reference analogue: src/erasor_dynamic.cpp:16-35 (the original points that no point of a remover's static map has as its nearest
 * neighbour are the dynamic cloud) and the evaluation block of SSC::segDF, ssc.cpp:1511-1540 (the same look-up from cloud_eva_static
 * into the labelled original cloud; the hit points, without those labelled 252, are the _static.pcd analysis.py reads).  It builds what
 * scvod_evaluate_device, scvod_classify_map_device and scvod_score_classes_device take when the cleaned cloud comes from outside.
 *   per query       its nearest base point over the WHOLE base cloud -- no radius -- by the squared distance d = (dx*dx + dy*dy) + dz*dz in
 *                   fp32 with dx = base.x - query.x (the evaluation's expression, no contraction), ties to the lowest base index; an
 *                   empty base gives index -1 and distance +inf.  The result does not depend on cell, on max_rings, on the order inside
 *                   a bucket or on which pass finished the query
 *   per base point  one byte: SCVOD_SPLIT_MISS when no query chose it; otherwise SCVOD_SPLIT_GATED when n_reject_classes > 0 and
 *                   (d_base_label[i] & 0xFFFF) is in reject_classes; otherwise SCVOD_SPLIT_HIT.  A function of the point alone, never of
 *                   how many queries chose it or in which order.  mark == SCVOD_SPLIT_HIT is scvod_classify_map_device's d_pred_static
 *   partition       the base indices of the HIT points ascending, then of the MISS points ascending, then of the GATED points ascending
 *                   (a stable three-way partition).  Without a reject list the MISS segment is erasor_dynamic.cpp's dynamic_cloud
 *                   (ExtractIndices, negative); with {252} the HIT segment is evaluate_static of ssc.cpp:1533-1534 (sampleVec: sort +
 *                   unique, so ascending too)
 * The look-up is a hash grid of cell edge `cell` over the base cloud in three passes: the 27 cells around a query (finished when its
 * candidate is closer than 0.99 cell edges), the rings 2 .. max_rings of cells (finished after ring r when closer than 0.99 r cell
 * edges), and for what is left an exhaustive scan of the base cloud, n_base records per such query: exact for any input, counted by
 * scvod_map_split_stats, and not a design target -- a cleaned map, where every query has a base point within a cell or two, never
 * reaches it.  All counters are integer sums and the partition is stable: the same bytes on every run. */
#define SCVOD_SPLIT_MISS 0   /* no query chose this base point                                   */
#define SCVOD_SPLIT_HIT 1    /* the nearest base point of at least one query                      */
#define SCVOD_SPLIT_GATED 2  /* hit, but its label & 0xFFFF is in reject_classes (ssc.cpp:1524)   */
typedef struct scvod_split_params {
    float cell;                  /* edge of the hash grid's cells; default 0.2; positive, finite  */
    int32_t max_rings;           /* last ring of cells the ring pass walks; default 3; 1..8       */
    int32_t base_stride;         /* floats per base record: 3 (packed xyz) or 4 (xyzi, 16-byte aligned); default 3 */
    int32_t query_stride;        /* the same for the query cloud; default 3                       */
    int32_t n_reject_classes;    /* 0..16; default 0 (erasor_dynamic.cpp); segDF's block: {252}   */
    uint16_t reject_classes[16];
} scvod_split_params;
/* cell 0.2, max_rings 3, both strides 3, no reject class */
void scvod_split_params_default(scvod_split_params* p);
/* d_base [n_base] and d_query [n_query] records of base_stride / query_stride floats; d_base_label [n_base] uint32, NULL exactly when
 * n_reject_classes == 0.  params NULL = the defaults; the struct is copied before the call returns.  Outputs, each optional (NULL):
 *   d_mark         [n_base] the byte above
 *   d_order        [n_base] int32: the partition
 *   d_seg4         four int64 ON THE DEVICE: {0, n_hit, n_hit + n_miss, n_base}, the bounds of the three segments -- a consumer on the
 *                  same stream needs no host read
 *   d_base_out     [n_base * base_stride] floats: the base records in the partition's order, bit for bit (with stride 4 the intensity
 *                  word travels: NaN payload bits survive); must not overlap d_base
 *   d_payload_out  [n_base] one uint32 per base point in that order, from d_payload_in [n_base] (e.g. SemanticKITTI labels)
 *   d_nn_idx, d_nn_sqdist  [n_query] the neighbour of every query and its squared distance
 * Every output holds exactly n_base (n_query) entries: there is no capacity argument and no overflow state.  Stream-ordered (stream
 * NULL = the ctx's stream), never synchronises with the host; each call overwrites the stats of the one before, and the split calls
 * of one ctx must be ordered among themselves (they share their scratch).  Argument errors (NULL ctx, negative sizes, a NULL array
 * of a non-empty cloud, a stride other than 3 or 4, a stride-4 pointer that is not 16-byte aligned, d_payload_out without
 * d_payload_in, d_base_out overlapping d_base, more than 16 classes, a reject list without labels, a cell that is not positive and
 * finite, max_rings outside 1..8) are SCVOD_ERR_INVALID before any device is looked for; non-finite coordinates are unspecified.
 * Scratch (the grid, 20 bytes per query for the lists of the second and third pass, a mark byte per base point, 24 bytes per
 * 2048-point tile, 8 stats words) is an allocation of its own, grow-only, freed by scvod_destroy and NOT part of scvod_arena_bytes,
 * scvod_evaluate_scratch_bytes or scvod_score_classes_scratch_bytes; no result of the last batch changes.  Only a call that needs more
 * than any before waits for the split in flight before it grows. */
int scvod_map_split_device(scvod_ctx* ctx, const float* d_base, const uint32_t* d_base_label, int32_t n_base, const float* d_query,
                           int32_t n_query, const scvod_split_params* params, uint8_t* d_mark, int32_t* d_order, int64_t* d_seg4,
                           float* d_base_out, const uint32_t* d_payload_in, uint32_t* d_payload_out, int32_t* d_nn_idx,
                           float* d_nn_sqdist, void* stream);
/* h_out8 = {n_hit, n_miss, n_gated, queries finished by the 27-cell pass, by the ring pass, by the exhaustive pass, 0, 0} of the last
 * scvod_map_split_device.  Synchronises that call's stream.  SCVOD_ERR_STATE before the first split. */
int scvod_map_split_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the split holds on this ctx (0 before the first call) */
int64_t scvod_map_split_scratch_bytes(scvod_ctx* ctx);
/* The same for clouds in host memory (what the host tool scvod_map_split calls: it links this library only): the clouds are uploaded,
 * split on the device and the outputs asked for (h_mark, h_order, h_seg4 [4], h_base_out; each may be NULL) downloaded.  Synchronous.
 * The device buffers live for the duration of the call. */
int scvod_map_split(scvod_ctx* ctx, const float* h_base, const uint32_t* h_base_label, int32_t n_base, const float* h_query,
                    int32_t n_query, const scvod_split_params* params, uint8_t* h_mark, int32_t* h_order, int64_t* h_seg4,
                    float* h_base_out);

/* ---- the recognised ground / building / tree classes against labelled truth, on the device (opt-in: nothing runs or is allocated
 * unless it is called) ----------------------------------------------------------------------------------------------------------------
 * Reference analogue: src/plotObject.cpp:87-146, the tool behind the per-class table of doc/note.txt:57-78.  Every ground-truth point
 * looks up its nearest estimate point (squared distance d = (dx*dx + dy*dy) + dz*dz in fp32, ties to the lowest estimate index).
 *   truth class     of (label & 0xFFFF): 0 ground, 1 building, 2 tree -- the three lists, tested in this order (check(),
 *                   plotObject.cpp:16-29) -- and 3 pd for a label in no list
 *   estimate class  at the neighbour, from its SCVOD_PT_* byte as scvod_batch_point_classes writes it: 1 ground (SCVOD_PT_GROUND),
 *                   2 building (SCVOD_PT_STATIC_BUILDING), 3 tree (SCVOD_PT_STATIC_OTHER), 0 other (every other byte: car, rejected,
 *                   unclustered, dynamic), 4 none (no neighbour) -- the colour test of plotObject.cpp:51-85 on SSC::saveSegCloud's colours
 *   rules           ground: P iff the neighbour is ground.  building: P iff building or tree.  tree: P iff tree or building.  pd: P iff
 *                   the neighbour is `other` or d > 0.5f (PCL hands out squared distances: 0.5 m^2, as the reference wrote it).  No
 *                   neighbour: N for the first three classes, P for pd
 * Two departures from the reference: the estimate's y is y (plotObject.cpp copies z into it), and a neighbour
 * counts only when d < max_dist * max_dist (product in fp32); a truth point without one has the estimate class `none`, which is a
 * column of its own in conf.  max_dist * max_dist > 0.5f is required, so the pd rule is exactly the reference's unbounded one.
 * The look-up is a hash grid of cell edge `cell` searched ring by ring with early exit, R = ceil(max_dist / (0.99 * cell)) rings at the
 * most (R <= 32 is required); its result is that of an exhaustive search inside max_dist.  All counts are integer sums: the same on
 * every run. */
typedef struct scvod_class_params {
    float max_dist;            /* neighbours are looked for inside this distance; default 0.75 */
    float cell;                /* grid cell edge; default 0.25 */
    int32_t n_ground, n_building, n_tree; /* 0..8 each */
    uint16_t ground[8], building[8], tree[8];
} scvod_class_params;
/* max_dist 0.75, cell 0.25, the lists of plotObject.cpp:3-5: 40,44,48,49,71,72 / 50,51,52,60 / 70,80,81 */
void scvod_class_params_default(scvod_class_params* p);
typedef struct scvod_class_result {
    int64_t conf[4][5];   /* truth class x estimate class at the neighbour */
    int64_t pd_far;       /* pd points whose neighbour is not `other` but lies at d > 0.5 (they have a neighbour: `none` is not counted) */
    int64_t num[4], P[4]; /* filled by scvod_class_finish: points and P points per truth class */
    float rate_P[4], rate_N[4];
} scvod_class_result;
/* Host only, no device.  conf_and_far: conf row-major, then pd_far.  num = the row sums; P = conf[0][1], conf[1][2] + conf[1][3],
 * conf[2][2] + conf[2][3], conf[3][0] + conf[3][4] + pd_far; rate_P = (float)P / (float)num and rate_N = (float)(num - P) / (float)num in
 * fp32 (plotObject.cpp:143-146).  num == 0 gives NaN: the reference prints `nan` there. */
void scvod_class_finish(const int64_t conf_and_far[21], scvod_class_result* out);
/* Ground truth (d_gt_xyz packed at 12 B per point as in scvod_evaluate_device, d_gt_label uint32) against an estimate cloud of the same
 * form with one SCVOD_PT_* byte per point -- the map-level form: export with scvod_batch_export_points plus d_src_out and gather the
 * bytes of scvod_batch_point_classes.  d_point_result: NULL, or one byte per gt point: bits 0-1 the truth class, bits 2-4 the estimate
 * class, bit 5 P.  Stream-ordered (stream NULL = the ctx's stream), never synchronises with the host; each call overwrites the counters
 * of the one before, and the scoring calls of one ctx must be ordered among themselves (they share their scratch; the evaluation's
 * scratch is another one, so the two families need no order between them).  Argument errors (NULL ctx, negative sizes, a NULL array
 * of a non-empty cloud, a list longer than 8, a cell or max_dist that is not positive and finite, max_dist * max_dist <= 0.5, more than
 * 32 rings) are SCVOD_ERR_INVALID before any device is looked for.  Scratch (the grid, 12 bytes per gt point for the list of the second
 * pass, 24 counter words; for the batch form also world xyz, a keep byte and a class byte per point and 12 floats per scan) is an
 * allocation of its own, grow-only, freed by scvod_destroy and NOT part of scvod_arena_bytes or scvod_evaluate_scratch_bytes; a call
 * that needs more than any before waits for the scoring in flight before it grows. */
int scvod_score_classes_device(scvod_ctx* ctx, const float* d_gt_xyz, const uint32_t* d_gt_label, int32_t n_gt, const float* d_est_xyz,
                               const uint8_t* d_est_class, int32_t n_est, const scvod_class_params* params, uint8_t* d_point_result,
                               void* stream);
/* The protocol of scvod_batch_evaluate for the ctx's last batch: truth is EVERY input point of the batch in the world frame (h_poses
 * [n_scans][6], the expression of scvod_batch_export_points, staged before the call returns) with its label d_gt_label [batch points];
 * the estimate is the points scvod_batch_export_points would keep with the same `flags` -- as a keep mask over the same world array --
 * each carrying its byte of scvod_batch_point_classes.  State rules and errors are those of scvod_batch_point_labels with the same
 * flags (SCVOD_MAP_NO_GROUND, SCVOD_MAP_NO_REJECTED, SCVOD_MAP_IGNORE_DYNAMIC; the part flags are refused).  No output of the batch
 * changes.  Stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_score_classes(scvod_ctx* ctx, const uint32_t* d_gt_label, const float* h_poses, int32_t flags, const scvod_class_params* params,
                              uint8_t* d_point_result, void* stream);
/* counts and rates (scvod_class_finish) of the last scvod_score_classes_device / scvod_batch_score_classes.  Synchronises that call's
 * stream.  SCVOD_ERR_STATE before the first scoring call. */
int scvod_score_classes_stats(scvod_ctx* ctx, scvod_class_result* out);
/* how many truth points of that call went on to the second pass (no candidate within 0.99 cell edges in the 27 cells around them): a
 * measure of cost, not a result.  Synchronises that call's stream.  Returns the count or a negative status. */
int64_t scvod_score_classes_pass2_queries(scvod_ctx* ctx);
/* bytes of device scratch the class scores hold on this ctx (0 before the first call) */
int64_t scvod_score_classes_scratch_bytes(scvod_ctx* ctx);

/* ---- object scores: removal per labelled object, from a device instance table (opt-in: nothing runs or is allocated unless it is
 * called) ----------------------------------------------------------------------------------------------------------------------------
 * Reference analogue: tool/plotIoU.py:70-84 plots, per sequence, the high-dynamic objects of the truth (HD_gt) and how many of them were
 * removed (HD_removed), the low-dynamic objects (LD_gt) and how many were retained (LD_retained).  The numbers are hard-coded there and no
 * program of the reference computes them: the object rule below is THIS PROJECT'S CONVENTION.  SemanticKITTI
 * labels carry what it needs -- label & 0xFFFF the class, label >> 16 the instance -- and scvod_evaluate_device / scvod_batch_evaluate
 * write one byte per truth point that says whether the point survived.  The device part groups the points by their 32-bit label and
 * counts per group: integer sums and a minimum, the same bytes on every run and for every order of the points. */
typedef struct scvod_instance { /* 32 bytes */
    uint32_t label;
    int32_t first_point;  /* lowest point index carrying this key */
    int64_t n_points;
    int64_t n_inlier;     /* bit 0 of the result byte */
    int64_t n_preserved;  /* bit 0 set and (bit 1 set) == (bit 2 set): analysis.py's rule (num_static_preserved + num_dynamic_preserved) */
} scvod_instance;
/* d_key [n] one uint32 per point (the truth labels; opaque to the device: every value is a legal key, 0 and 0xFFFFFFFF included);
 * d_point_result [n] the bytes of scvod_evaluate_device / scvod_batch_evaluate (only bits 0-2 are read).  d_instances [cap_instances]
 * receives one record per distinct key, ascending by key; NULL counts only.  d_n [1] receives the record count ON THE DEVICE -- a
 * consumer on the same stream needs no host read.  cap_instances (1 .. 1 << 22) sizes the output and the global hash table (a power of
 * two of slots, at least 2 * cap_instances).  More distinct keys than cap_instances is an overflow: nothing is written at or behind
 * cap_instances, d_n[0] = -1, and the records inside the buffer are unspecified.  Stream-ordered, never synchronises with the host;
 * stream NULL = the stream of the ctx's last scvod_evaluate_device / scvod_batch_evaluate (the call whose bytes it reads), or the ctx's
 * stream when there was none.  Each call overwrites the stats of the one before, and the calls of one ctx must be ordered among
 * themselves (they share their scratch).  Argument errors (NULL ctx, n < 0 or n > INT32_MAX, a NULL array with n > 0, cap_instances
 * outside 1 .. 1 << 22, d_n NULL, d_instances or d_n not 8-byte aligned) are SCVOD_ERR_INVALID before any device is looked for.
 * Scratch (40 bytes per table slot, 24 bytes per record for the sort and its temporary storage, 8 counter words) is an allocation of
 * its own, grow-only, freed by scvod_destroy and NOT part of scvod_arena_bytes, scvod_evaluate_scratch_bytes or
 * scvod_score_classes_scratch_bytes; a call that needs more than any before waits for the one in flight before it grows. */
int scvod_score_instances_device(scvod_ctx* ctx, const uint32_t* d_key, const uint8_t* d_point_result, int64_t n, scvod_instance* d_instances,
                                 int32_t cap_instances, int64_t* d_n, void* stream);
/* h_out4 = {records written (counting only: that would have been), distinct keys found, overflow, tiles whose on-chip table spilled} of
 * the last scvod_score_instances_device.  Synchronises that call's stream.  After an overflow h_out4 is filled ("distinct keys found" is
 * then a lower bound, records written 0) and the call returns SCVOD_ERR_CAPACITY.  SCVOD_ERR_STATE before the first call. */
int scvod_score_instances_stats(scvod_ctx* ctx, int64_t* h_out4);
/* bytes of device scratch the object scores hold on this ctx (0 before the first call) */
int64_t scvod_score_instances_scratch_bytes(scvod_ctx* ctx);
/* Development switch behind profiles/instance_score_cost.txt, never needed for a result: 0 (the default) combines the equal keys of a
 * wave before they reach the on-chip table; 1 lets every point add into the on-chip table on its own.  The tables are identical. */
int scvod_set_score_instances_variant(scvod_ctx* ctx, int32_t variant);
typedef struct scvod_instance_params {
    int32_t n_dynamic_classes;    /* 0..16 */
    uint16_t dynamic_classes[16]; /* classes (label & 0xFFFF) of high-dynamic objects; default 252..259 */
    int32_t n_static_classes;     /* 0..16 */
    uint16_t static_classes[16];  /* classes of low-dynamic objects; default 10, 31, 30, 32, 16, 13, 18, 20 */
    double removed_below;         /* an HD object is removed iff n_preserved < removed_below * n_points; default 0.5 */
    double retained_from;         /* an LD object is retained iff n_preserved >= retained_from * n_points; default 0.5 */
    int64_t min_points;           /* smaller records are skipped; default 1 */
} scvod_instance_params;
/* dynamic classes 252..259; static classes 10, 31, 30, 32, 16, 13, 18, 20 (the SemanticKITTI static counterparts of 252..259 in that
 * order: car, bicyclist, person, motorcyclist, on-rails, bus, truck, other-vehicle); both thresholds 0.5; min_points 1 */
void scvod_instance_params_default(scvod_instance_params* p);
typedef struct scvod_instance_result {
    int64_t hd_gt, hd_removed, ld_gt, ld_retained;
    int64_t hd_points, hd_points_preserved, ld_points, ld_points_preserved;
    int64_t skipped;
    double hd_removed_rate, ld_retained_rate; /* 100.0 * hd_removed / hd_gt and 100.0 * ld_retained / ld_gt; NaN for a zero denominator */
} scvod_instance_result;
/* Host only, no device.  A record is an object iff label >> 16 != 0, n_points >= min_points and its class is in one of the two lists
 * (dynamic wins when it is in both); every other record counts in `skipped`.  The products are taken in double:
 * (double)n_preserved < removed_below * (double)n_points, (double)n_preserved >= retained_from * (double)n_points.  params NULL = the
 * defaults.  SCVOD_ERR_INVALID: a NULL table with n > 0, n < 0, out NULL, a list length outside 0..16, a threshold that is not finite. */
int scvod_instance_finish(const scvod_instance* table, int64_t n, const scvod_instance_params* params, scvod_instance_result* out);
/* Host only.  Two tables ascending by key -> one (the batches or shards of one sequence scored together): counts are added, first_point
 * is the smaller of the two.  *n_out is the true size; SCVOD_ERR_CAPACITY when it exceeds cap (nothing is written behind cap; out may
 * be NULL with cap 0: count only).  SCVOD_ERR_INVALID for an input that is not strictly ascending (nothing is written then). */
int scvod_instance_merge(const scvod_instance* a, int64_t na, const scvod_instance* b, int64_t nb, scvod_instance* out, int64_t cap,
                         int64_t* n_out);

/* ---- the truth label every object of the table covers, on the device (opt-in: nothing runs or is allocated unless it is called) ----
 * Reference analogue: none.  tool/feature.py (per-class feature boxplots) and tool/plotIoU.py (object counts) hold hard-coded numbers;
 * no program of the reference joins Frame::cluster_set with labelled truth.  The device part is a group-by with integer counts and is
 * exact; the object rule on the host (scvod_object_truth_finish) is THIS PROJECT'S CONVENTION.  A member point's
 * label is d_gt_label[scan_offsets[s] + apri_src[slot]] -- the join d_member_src documents; label & 0xFFFF is its class, label >> 16
 * its instance, and every 32-bit value is a legal label, 0 and 0xFFFFFFFF included.  One record per object, in table order; `label` is
 * the key of scvod_instance, so a record joins with the instance table on the host.  The records are the same bytes on every run and
 * depend on the multiset of an object's labels alone. */
#define SCVOD_OBJ_TRUTH_ONCHIP_LABELS 128 /* an object with at most this many distinct labels never takes the fallback path */
typedef struct scvod_object_truth { /* 32 bytes */
    uint32_t label;      /* the 32-bit truth label most members carry; equal counts: the SMALLEST label value                */
    int32_t n_label;     /* members carrying it                                                                              */
    int32_t n_class;     /* members whose (l & 0xFFFF) == (label & 0xFFFF)                                                   */
    int32_t n_moving;    /* members whose (l & 0xFFFF) is in params->dynamic_classes                                         */
    int32_t n_distinct;  /* distinct 32-bit labels among the members                                                         */
    int32_t n_points;    /* members (== scvod_object::n_points)                                                              */
    int32_t reserved[2]; /* 0                                                                                                */
} scvod_object_truth;
/* One scvod_object_truth per object of the LAST scvod_batch_objects call of this batch that asked for records, members or the
 * per-point objects, into d_truth [cap_truth]: the call reads the sorted member list that call left in the table's scratch, exactly as
 * scvod_batch_object_shapes does, under the same state rules (SCVOD_ERR_STATE without such a call -- a count-only call is none -- or
 * after another clustering; SCVOD_ERR_STATE without clustering and types of the batch; SCVOD_ERR_INVALID when the table read a tracking
 * result that is stale now; a SCVOD_OBJ_NO_TRACK table is fine).  d_gt_label: the array scvod_batch_evaluate takes, one uint32 per
 * INPUT point of the last batch.  params: only n_dynamic_classes / dynamic_classes are read (NULL: scvod_eval_params_default).
 * Stream-ordered (stream NULL = the stream of the ctx's last batch call; the table call must be ordered before it), never synchronises
 * with the host; each call overwrites the stats of the one before, and the calls of one ctx must be ordered among themselves (they
 * share their scratch).  Argument errors (NULL ctx, d_gt_label or d_truth NULL or not 4-byte aligned, cap_truth < 0, a class count
 * outside 0..16) are SCVOD_ERR_INVALID before any device is looked for.  Nothing is written at or behind cap_truth; the overflow is
 * latched until the next call.  An object with more than SCVOD_OBJ_TRUTH_ONCHIP_LABELS distinct labels is counted again in global
 * memory by a second launch on the same stream (32 workgroups, none of which waits for another); its record is the same.  Scratch
 * (4 bytes per 129 batch points for the list of such objects, 32 regions of 16 bytes per point of the batch's largest scan, 8 counter
 * words) is an allocation of its own, grow-only, freed by scvod_destroy and NOT part of scvod_arena_bytes or
 * scvod_batch_objects_scratch_bytes; a call that needs more than any before waits for the one in flight before it grows. */
int scvod_batch_object_truth(scvod_ctx* ctx, const uint32_t* d_gt_label, const scvod_eval_params* params, void* d_truth, int64_t cap_truth,
                             void* stream);
/* h_out8 = {records written, objects of the table, 1 when the table outgrew cap_truth, objects that took the fallback path, input
 * points of the batch whose class is in the list, the sum of n_moving over ALL objects of the table (those at or behind cap_truth
 * too), 0, 0} of the last scvod_batch_object_truth: word 4 minus word 5 is the number of moving points that sit in no object at all.
 * Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow (h_out8 is filled), SCVOD_ERR_STATE before the first call. */
int scvod_batch_object_truth_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the stage holds on this ctx (0 before the first call) */
int64_t scvod_batch_object_truth_scratch_bytes(scvod_ctx* ctx);
typedef struct scvod_object_truth_params {
    double moving_from; /* an object is truth-moving iff n_moving >= moving_from * n_points; default 0.5 */
    double pure_from;   /* an object is mixed iff n_label < pure_from * n_points; default 0.5            */
    int64_t min_points; /* smaller objects are skipped; default 1                                        */
} scvod_object_truth_params;
/* 0.5, 0.5, 1 */
void scvod_object_truth_params_default(scvod_object_truth_params* p);
typedef struct scvod_object_truth_result {
    int64_t moving_objects;       /* truth-moving objects: the sum of the next four                                           */
    int64_t moving_dynamic;       /* ... with dynamic == 1: found                                                             */
    int64_t moving_car_static;    /* ... not dynamic, cls == 2, state == 0: walked by the tracking and judged static          */
    int64_t moving_car_untracked; /* ... not dynamic, cls == 2, any other state (-1 in a table): typed car, never judged      */
    int64_t moving_not_car;       /* ... not dynamic, cls != 2: typed tree or building, so the tracking never walked it       */
    int64_t static_objects;       /* the other objects                                                                        */
    int64_t static_dynamic;       /* ... with dynamic == 1: false alarms                                                      */
    int64_t mixed_objects;        /* objects of either kind whose winning label covers less than pure_from of their members   */
    int64_t skipped;              /* objects below min_points (counted nowhere else)                                          */
    double precision;             /* 100.0 * moving_dynamic / (moving_dynamic + static_dynamic); NaN for a zero denominator   */
    double recall;                /* 100.0 * moving_dynamic / moving_objects; NaN for a zero denominator                      */
} scvod_object_truth_result;
/* Host only, no device.  objects [n] and truth [n]: the records of one table and of the truth call on it, index by index.  The
 * products are taken in double: (double)n_moving >= moving_from * (double)n_points, (double)n_label < pure_from * (double)n_points,
 * with n_points of the truth record.  params NULL = the defaults.  SCVOD_ERR_INVALID: a NULL array with n > 0, n < 0, out NULL, a
 * threshold that is not finite. */
int scvod_object_truth_finish(const scvod_object* objects, const scvod_object_truth* truth, int64_t n, const scvod_object_truth_params* params,
                              scvod_object_truth_result* out);

/* ---- scan stacking: neighbouring scans moved into the middle scan's frame, on the device (opt-in: nothing runs or is allocated
 * unless it is called) -------------------------------------------------------------------------------------------------------------
 * Reference analogue: src/makeScan.cpp:153-244, the stacker in front of the path for sparse, non-repetitive sensors.  Output scan
 * ("group") g is built from the `window` consecutive input scans g * interval .. g * interval + window - 1: the MIDDLE scan
 * mid = g * interval + window / 2 first, its records bit for bit (the reference never transforms cloud2), then the other scans of the
 * window in ascending scan index, each in input order, each point moved by T = scvod_pose_delta(pose_k, pose_mid) (trans_mid^-1 *
 * trans_k, makeScan.cpp:187-188) with T0*x + T1*y + T2*z + T3 per row, evaluated left to right in fp32 without contraction (the map
 * kernel's expression; makeScan.cpp:83-85); the intensity word is copied bit for bit.  The group hands on the middle scan's pose.
 * Group g exists iff g * interval + window <= n_in; with SCVOD_STACK_REFERENCE_BOUND also g * interval < n_in - interval, the loop
 * bound of makeScan.cpp:156 (`i < size - interval`), which drops the last complete group when n_in is a multiple of interval.
 * n_in < window gives no group (the reference's unsigned underflow there is not modelled).  window is odd, 1..9 (the reference: 3);
 * interval >= 1 (the reference: 3); interval < window stacks overlapping windows. */
#define SCVOD_STACK_REFERENCE_BOUND 1
#define SCVOD_STACK_MAX_WINDOW 9
/* Host only, no device.  Returns the number of groups n_out, or a negative status.  h_in_offsets [n_in + 1] point offsets of the input
 * scans (may be NULL when neither h_out_offsets nor largest_scan is asked for); h_out_offsets [n_out + 1] the point offsets of the
 * stacked scans; h_mid [n_out] the middle scan of every group; *largest_scan the largest stacked scan (to be checked against
 * SCVOD_MAX_SCAN_POINTS before scvod_batch_process).  Any of the three may be NULL: count only.  cap_out: the groups h_out_offsets
 * (cap_out + 1 words) and h_mid hold -- SCVOD_ERR_CAPACITY when a non-NULL array is too small, and when the stacked points outgrow
 * int32 offsets.  SCVOD_ERR_INVALID for a window that is even or outside 1..9, interval < 1, an unknown flag bit, n_in < 0 or
 * offsets that decrease. */
int scvod_stack_offsets(const int32_t* h_in_offsets, int32_t n_in, int32_t window, int32_t interval, int32_t flags,
                        int32_t* h_out_offsets, int32_t* h_mid, int32_t cap_out, int32_t* largest_scan);
/* Host only.  Row-major 3x4 in, {x, y, z, roll, pitch, yaw} out: rotationMatrixToEulerAngles of makeScan.cpp:57-74 with the float
 * overloads of sqrt / atan2 (sy < 1e-6, compared in double, takes the singular branch: yaw 0) and the translation column, as
 * makeScan.cpp:164-183 fills the pose it hands on.  scvod_pose_matrix of the result is the matrix the reference stacks with. */
void scvod_pose_from_matrix(const float M[12], float pose_out[6]);
/* The stacking on scans resident in HBM.  d_xyzi_in: all input scans concatenated (h_in_offsets [n_in + 1], starting anywhere:
 * point index h_in_offsets[k] + i is record h_in_offsets[k] + i of d_xyzi_in); h_poses [n_in][6].  Outputs, all in the order above:
 *   d_xyzi_out     [cap_points] packed float4 records
 *   d_payload_out  [cap_points] or NULL: one uint32 per point (e.g. SemanticKITTI labels for the evaluation calls) carried along from
 *   d_payload_in   [input points] or NULL
 *   d_src_out      [cap_points] or NULL: the input index h_in_offsets[k] + i of every output point
 * Stream-ordered (stream NULL = the ctx's stream), never synchronises with the host.  h_in_offsets and h_poses are turned into matrices
 * and a segment / tile table and staged before the call returns: the arrays are the caller's again at once (a later call with other
 * values waits for the staging copy in flight only when it needs the same staging slot again).  The stacking calls of one ctx must be
 * ordered among themselves (they share the table's device copy).  Unlike scvod_batch_voxelgrid the call does NOT invalidate the results
 * of the last batch: it touches neither the arena nor any batch state.  Scratch (64 bytes per segment, 8 bytes per 2048-point tile) is a
 * grow-only allocation of its own, freed by scvod_destroy, NOT part of scvod_arena_bytes, and does not exist before the first call.
 * Refused before anything is launched: SCVOD_ERR_INVALID for a bad window / interval / flag bit, offsets that decrease or start below
 * 0, a NULL array that is needed, a pointer that is not 16-byte (xyzi) or 4-byte (payload, src) aligned, d_payload_out without
 * d_payload_in, and an output range that overlaps its input range; SCVOD_ERR_CAPACITY when the stacked points exceed cap_points (the
 * host knows the size from the offsets: nothing is ever written at or behind the capacity).  No group (n_out == 0) is success and
 * launches nothing.  The sizes are scvod_stack_offsets' with the same arguments. */
int scvod_batch_stack_scans(scvod_ctx* ctx, const void* d_xyzi_in, const int32_t* h_in_offsets, int32_t n_in, const float* h_poses,
                            int32_t window, int32_t interval, int32_t flags, const uint32_t* d_payload_in, void* d_xyzi_out,
                            uint32_t* d_payload_out, int32_t* d_src_out, int64_t cap_points, void* stream);
/* The same for scans in host memory (what the C++ facade calls: it links this library only): the clouds are uploaded, stacked on the
 * device and downloaded into h_xyzi_out [cap_points]; h_xyzi_in holds the scans' records at their offsets.  Synchronous.  The device
 * buffers live for the duration of the call. */
int scvod_stack_scans(scvod_ctx* ctx, const float* h_xyzi_in, const int32_t* h_in_offsets, int32_t n_in, const float* h_poses,
                      int32_t window, int32_t interval, int32_t flags, float* h_xyzi_out, int64_t cap_points);
/* bytes of device scratch the stacking holds on this ctx (0 before the first call) */
int64_t scvod_stack_scratch_bytes(scvod_ctx* ctx);

/* ---- seen-through points: the range-image vote of neighbouring scans, on the device (opt-in: nothing runs or is allocated unless it
 * is called) ---------------------------------------------------------------------------------------------------------------------------
 * Reference analogue: none.  THIS PROJECT'S CONVENTION: SSC::tracking decides "dynamic" for car-typed clusters
 * only; this stage adds free-space evidence for ANY point.  If a neighbouring scan measures a return well behind the place where this
 * scan saw a point, a ray passed through that place and it was empty then.
 *
 * Grid and depth: the ctx's own binning.  A pixel is (azimuth_idx, sector_idx), A = azimuth_num rows by S = sector_num columns; the
 * depth is PointAPRI::range, the 2-D distance `dis` of SSC::makeApriVec.  The range image of scan s, img[s][ai * S + si], is the
 * minimum `dis` over the scan's input points whose x, y, z are finite, which pass makeApriVec's range / FOV test and whose indices lie
 * in 0 <= si < S, 0 <= ai < A.  EVERY input point takes part, ground and Patchwork-dropped ones included: a ray that ends on the road
 * behind an object is evidence.  A pixel without such a point holds +inf (0x7F800000).  The image is an integer minimum over the float
 * bits: order-independent, the same on every run.
 *
 * Viewers of scan j: up to `after` successors along h_next_scan (the table of scvod_batch_track: NULL means s + 1, and the last scan has
 * none; a negative entry -- none, or an external table -- ends the chain inside the batch) and up to `before` predecessors along the
 * inverse of that table.  Scans at the ends of a chain have fewer viewers; interleaved chains follow from the table.  A table in which
 * two scans name one successor, a scan names itself, the chain closes into a ring, or an entry is >= n_scans is refused.
 *
 * One pair (query point q of scan j, viewer s): T = scvod_pose_delta(pose_j, pose_s) moves a point of j's frame into s's frame
 * (trans_s^-1 * trans_j); p' = T q with T0*x + T1*y + T2*z + T3 per row, left to right in fp32 without contraction (the map, export and
 * stack kernels' expression); dis', si, ai and keep are makeApriVec's of p'.  The pair's class is the first that applies:
 *   OUTSIDE   p' is not finite, keep == 0, or an index lies outside the image
 *   otherwise, over the window [ai - halo, ai + halo] x [si - halo, si + halo] clipped to the image -- NO wrap across the sector seam
 *   (the reference's neighbourhoods do not wrap there either) -- with gap = gap_abs + gap_rel * dis' (fp32, two operations) and r_min
 *   the minimum of the window:
 *   EMPTY     r_min == +inf
 *   THROUGH   r_min > dis' + gap (strict: every return of the window lies behind the point)
 *   AGREE     some pixel r of the window has fabsf(r - dis') <= gap
 *   OCCLUDED  otherwise
 * Per query point one uint32 of four byte counters: byte 0 n_through, byte 1 n_agree, byte 2 n_occluded, byte 3 n_outside + n_empty;
 * they sum to the viewer count of the point's scan.  A point that is no query gets 0.  The verdict byte:
 *   SCVOD_VIS_UNTESTED      not a query, or a scan without viewers
 *   SCVOD_VIS_SEEN_THROUGH  n_through >= min_through && n_through * vote_den >= vote_num * (n_through + n_agree), in int
 *   SCVOD_VIS_KEEP          every other query
 * The intended use: scvod_batch_visibility, then scvod_map_accumulate_labelled with the verdict bytes as labels and a keep table that
 * holds everything but SCVOD_VIS_SEEN_THROUGH. */
#define SCVOD_VIS_UNTESTED 0
#define SCVOD_VIS_KEEP 1
#define SCVOD_VIS_SEEN_THROUGH 2
#define SCVOD_VIS_WITH_GROUND 1 /* scvod_batch_visibility: every input point is a query, not only Patchwork's non-ground list */
#define SCVOD_VIS_IMAGES_ONLY 2 /* scvod_batch_visibility: the range images only (into d_images or the scratch): no vote, no other output */
#define SCVOD_VIS_MAX_WINDOW 32 /* viewers on each side */
typedef struct scvod_visibility_params { /* 32 bytes */
    int32_t before, after; /* viewers on each side: 0..SCVOD_VIS_MAX_WINDOW each, not both 0 */
    int32_t halo;          /* 0 or 1: the window is (2 halo + 1)^2 pixels                    */
    float gap_abs;         /* metres, >= 0 and finite                                        */
    float gap_rel;         /* per metre of dis', >= 0 and finite                             */
    int32_t min_through;   /* any value                                                      */
    int32_t vote_num;      /* 0 .. 1 << 20                                                   */
    int32_t vote_den;      /* 1 .. 1 << 20                                                   */
} scvod_visibility_params;
/* before = after = 2, halo 0, gap_abs 0.4f, gap_rel 0.02f, min_through 2, vote 1 / 2.  These values come from a float64 prototype of
 * the rule on the synthetic scans of this repository, NOT from real data. */
void scvod_visibility_params_default(scvod_visibility_params* p);
/* Host only, no device: the viewer lists the two calls below use.  h_next_scan [n_scans] or NULL.  h_begin [n_scans + 1] receives the
 * first viewer of every scan in h_viewers [cap]: per scan the successors, nearest first, then the predecessors, nearest first.  Either
 * array may be NULL (count only).  Returns the number of (scan, viewer) pairs, SCVOD_ERR_INVALID for n_scans < 0, a window outside
 * 0..SCVOD_VIS_MAX_WINDOW or 0 on both sides, or a table refused above, SCVOD_ERR_CAPACITY when h_viewers is too small. */
int scvod_visibility_viewers(const int32_t* h_next_scan, int32_t n_scans, int32_t before, int32_t after, int32_t* h_begin,
                             int32_t* h_viewers, int32_t cap);
/* The vote on any cloud of 16-byte records resident in HBM.  d_xyzi, h_scan_offsets [n_scans + 1] and h_poses [n_scans][6] as
 * scvod_map_query takes them (NULL poses: the zero pose for every scan; offsets ascending, starting at or above 0); every per-point
 * array is indexed like d_xyzi.  d_query_mask: one byte per point, != 0 is a query; NULL: every point.  Outputs, each may be NULL:
 *   d_votes       one uint32 per point (the four byte counters)
 *   d_verdict     one byte per point
 *   d_images      [n_scans][A * S] floats, the range images; without it they live in the stage's scratch
 *   d_scan_counts [n_scans][6] int64 {queries, SEEN_THROUGH, pairs THROUGH, AGREE, OCCLUDED, OUTSIDE + EMPTY}
 * Stream-ordered (stream NULL = the ctx's stream), never synchronises with the host; h_scan_offsets, h_poses and h_next_scan are
 * turned into tile, scan and pair tables -- the matrices of all (scan, viewer) pairs come from scvod_pose_delta on the host -- and
 * staged before the call returns.  The call touches neither the arena nor any batch state.  Integer counts and minima only: every
 * output is bit-identical from run to run.  Each call overwrites the stats of the one before, and the calls of one ctx must be
 * ordered among themselves (they share their scratch).  Argument errors (NULL ctx or params, n_scans < 0, NULL offsets with
 * n_scans > 0, offsets that decrease or start below 0, a window outside 0..32 or 0 on both sides, halo outside 0..1, vote_den outside
 * 1 .. 1 << 20, vote_num outside 0 .. 1 << 20, a negative or non-finite gap, a successor table refused above, a NULL cloud that is not
 * empty, d_xyzi or d_images not 16-byte, d_votes not 4-byte, d_scan_counts not 8-byte aligned) are SCVOD_ERR_INVALID before any device
 * is looked for.  Scratch (4 A S bytes per scan for the images unless d_images is given -- 72 KB per scan of the SemanticKITTI grid,
 * 288 KB of the OS1-128 grid --, 64 bytes per (scan, viewer) pair, 16 bytes per scan, 8 bytes per 2048-point tile, in the batch form a
 * mask byte per point, 8 counter words) is a grow-only allocation of its own, freed by scvod_destroy and NOT part of
 * scvod_arena_bytes; a call that needs more than any before waits for the one in flight before it grows. */
int scvod_visibility_device(scvod_ctx* ctx, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                            const int32_t* h_next_scan, const uint8_t* d_query_mask, const scvod_visibility_params* params,
                            uint32_t* d_votes, uint8_t* d_verdict, float* d_images, int64_t* d_scan_counts, void* stream);
/* The same for the input cloud of the ctx's last batch.  Queries are the points of Patchwork's non-ground list (the three index lists
 * are written first when a lean batch left them out; a mask is scattered into the stage's scratch), or with SCVOD_VIS_WITH_GROUND
 * every input point.  Needs scvod_batch_process only (with Patchwork, unless SCVOD_VIS_WITH_GROUND; on an input cloud), otherwise
 * SCVOD_ERR_STATE: clustering, types and tracking are not needed and not touched.  h_poses [n_scans][6] (NULL: the zero pose).
 * With SCVOD_VIS_IMAGES_ONLY the call stops after the range images: d_votes, d_verdict and d_scan_counts must be NULL, no list is
 * needed, and the stats of the call are all 0.  Stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_visibility(scvod_ctx* ctx, const float* h_poses, const int32_t* h_next_scan, const scvod_visibility_params* params,
                           int32_t flags, uint32_t* d_votes, uint8_t* d_verdict, float* d_images, int64_t* d_scan_counts, void* stream);
/* h_out8 = {queries, SEEN_THROUGH, pairs THROUGH, AGREE, OCCLUDED, OUTSIDE + EMPTY, (query, viewer) pairs, 0} of the last vote.
 * Synchronises that call's stream.  SCVOD_ERR_STATE before the first call. */
int scvod_visibility_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the vote holds on this ctx (0 before the first call) */
int64_t scvod_visibility_scratch_bytes(scvod_ctx* ctx);

/* ---- a world-frame cloud against the range images of every scan in reach (csrc/scvod_cloudvis.hip) ----
 * Reference analogue: none; this project's convention, the map-level step of Removert / ERASOR-style cleaners.
 * The vote above looks at a point of scan j from a few scans along the successor table.  Here the query is ANY cloud in the world
 * frame -- the representatives of a static map (scvod_map_points), a merged map, a scan moved to the world -- and EVERY scan of the
 * call is a viewer of every point; there is no successor table.
 *   d_xyzi    n 16-byte records in the world frame; the intensity word is ignored
 *   d_images  [n_scans][A * S] floats, exactly what scvod_visibility_device / scvod_batch_visibility write on this ctx's grid
 *             (SCVOD_VIS_IMAGES_ONLY writes them alone)
 *   h_poses   [n_scans][6]; NULL: the zero pose for every scan
 * The viewer of a pair is scan s: T_s = scvod_pose_delta(zero pose, pose_s), that is trans_s^-1, computed on the host as the scan stage
 * computes its matrices; p' = T_s q with T0*x + T1*y + T2*z + T3 per row, left to right in fp32 without contraction.  The pair's class
 * is the rule stated above on p' (one device function serves both stages), with its OUTSIDE / EMPTY cases told apart -- OUTSIDE, EMPTY,
 * THROUGH, AGREE, OCCLUDED -- and one addition: with max_range > 0 a pair with dis' > max_range is OUTSIDE.
 *   d_votes[i][4]  uint16 counters {n_through, n_agree, n_occluded, n_empty} of point i.  OUTSIDE pairs are not counted (on a
 *                  trajectory they are nearly all pairs).  n_scans <= 65535, so no counter can wrap.
 *   d_verdict[i]   SCVOD_VIS_UNTESTED      iff the record is not finite or all four counters are 0
 *                  SCVOD_VIS_SEEN_THROUGH  iff n_through >= min_through &&
 *                                          (int64)n_through * vote_den >= (int64)vote_num * (n_through + n_agree)
 *                  SCVOD_VIS_KEEP          otherwise
 * Either output may be NULL.  Every output is an integer count: it does not depend on the order of the points or of the work and is
 * bit-identical from run to run.  The intended use: scvod_batch_visibility with SCVOD_VIS_IMAGES_ONLY, scvod_map_points, this call,
 * then scvod_map_accumulate_labelled of the same points with the verdict bytes as labels and a keep table without
 * SCVOD_VIS_SEEN_THROUGH: the cleaned map is a new labelled map.
 * How it runs: the points are keyed by a 2 m world tile (x, y interleaved; records that are not finite and tiles beyond +-16.384 km
 * share the last key, which costs time, never correctness), (key, index) pairs are radix-sorted on the 28 key bits, and a workgroup
 * walks all scans for 512 consecutive sorted points, skipping a scan when no point of its chunk can lie within the reach
 * min(max_dis, max_range) of that sensor (the bound: DESIGN.md section 2).  The skip changes no output bit.  SCVOD_CVIS_NO_SORT leaves
 * the sort out and cuts the chunks from the input order: identical outputs, for a cloud that already is spatially coherent (a scan)
 * and for measuring what the sort buys.
 * Stream-ordered (stream NULL = the ctx's stream), never synchronises with the host; h_poses is turned into matrices and staged before
 * the call returns.  The call touches neither the arena nor any batch state nor the scan stage's scratch or stats.  Each call
 * overwrites the stats of the one before, and the calls of one ctx must be ordered among themselves (they share their scratch).
 * Argument errors (NULL ctx or params, n < 0, n_scans < 0 or > 65535, reserved != 0, a parameter outside the ranges below, NULL
 * d_images with n_scans > 0, a NULL cloud with n > 0, d_xyzi or d_images not 16-byte aligned, d_votes not 8-byte aligned, unknown flag
 * bits) are SCVOD_ERR_INVALID before any device is looked for; n > 2^31 - 1 is SCVOD_ERR_CAPACITY.  n == 0 or n_scans == 0 is fine:
 * every finite point is UNTESTED.  Scratch (48 bytes per scan; with the sort 16 bytes per point and rocprim's temporary storage; 10
 * counter words) is a grow-only allocation of its own, freed by scvod_destroy and NOT part of scvod_arena_bytes; a call that needs
 * more than any before waits for the one in flight before it grows. */
typedef struct scvod_cloud_visibility_params { /* 32 bytes */
    int32_t halo;        /* 0 or 1: the window is (2 halo + 1)^2 pixels                     */
    float gap_abs;       /* metres, >= 0 and finite                                         */
    float gap_rel;       /* per metre of dis', >= 0 and finite                              */
    float max_range;     /* metres, >= 0 and finite; 0: the grid's max_dis alone            */
    int32_t min_through; /* any value                                                       */
    int32_t vote_num;    /* 0 .. 1 << 20                                                    */
    int32_t vote_den;    /* 1 .. 1 << 20                                                    */
    int32_t reserved;    /* 0                                                               */
} scvod_cloud_visibility_params;
#define SCVOD_CVIS_NO_SORT 1 /* chunks of consecutive INPUT points: no key, no sort; outputs identical */
/* halo 0, gap_abs 0.4f, gap_rel 0.02f, max_range 0, min_through 2, vote 1 / 2: the scan stage's values.  They are NOT tuned for maps
 * (a map point has hundreds of viewers, a scan point four) and NOT from real data. */
void scvod_cloud_visibility_params_default(scvod_cloud_visibility_params* p);
int scvod_cloud_visibility_device(scvod_ctx* ctx, const void* d_xyzi, int64_t n, const float* d_images, const float* h_poses,
                                  int32_t n_scans, const scvod_cloud_visibility_params* params, int32_t flags, uint16_t* d_votes,
                                  uint8_t* d_verdict, void* stream);
/* h_out10 = {points, finite records, SEEN_THROUGH, KEEP, UNTESTED among the finite, pairs THROUGH, AGREE, OCCLUDED, EMPTY, (chunk, scan)
 * steps that were not skipped} of the last call.  Word 9 depends on the implementation (chunk size, order, bound); it is at most
 * ceil(n / 512) * n_scans.  Synchronises that call's stream.  SCVOD_ERR_STATE before the first call. */
int scvod_cloud_visibility_stats(scvod_ctx* ctx, int64_t* h_out10);
/* bytes of device scratch the stage holds on this ctx (0 before the first call) */
int64_t scvod_cloud_visibility_scratch_bytes(scvod_ctx* ctx);

/* ---- the objects of a batch vote on the seen-through verdict (opt-in: nothing runs unless it is called; csrc/scvod_objvis.hip) ----
 * Reference analogue: none.  No program of the reference joins free-space evidence with its clusters; the rule and both sets of
 * defaults are this project's convention, and the defaults are NOT from real data.
 * scvod_batch_visibility answers per point: the half of a moving car that no neighbouring scan looks behind stays KEEP or UNTESTED, and
 * a few strays of a wall come out SEEN_THROUGH.  This call joins the verdict bytes with the object table: per object of the table the
 * last scvod_batch_objects left in the ctx's scratch (the state rules and SCVOD_ERR_STATE cases of scvod_batch_object_truth; a
 * SCVOD_OBJ_NO_TRACK table is fine), over its members -- the input points d_member_src lists --
 *   n_seen / n_keep / n_untested   members whose byte of d_verdict is 2 / 1 / anything else
 *   sum_through .. sum_other       bytes 0..3 of d_votes summed over ALL members (0 without d_votes)
 * With t = n_seen, a = n_keep (SCVOD_OBJVIS_POOL_PAIRS: t = sum_through, a = sum_agree) an object VOTES iff
 *   n_points >= min_points && n_keep + n_seen >= min_tested
 * and its verdict is SCVOD_VIS_SEEN_THROUGH iff
 *   t >= min_through && (int64)t * vote_den >= (int64)vote_num * ((int64)t + a)
 * and SCVOD_VIS_KEEP otherwise (how = 1).  With SCVOD_OBJVIS_WITH_TRACK an object whose record in d_objects has dynamic == 1 is
 * SCVOD_VIS_SEEN_THROUGH with how = 2 whether or not it votes: voxel differencing speaks for car-typed clusters, free space for
 * anything.  Every other object has verdict -1, how 0.  Integers only: host and device agree by construction, and every output is
 * bit-identical from run to run.
 *   d_verdict      one byte per INPUT point of the ctx's last batch, what scvod_batch_visibility wrote; any bytes are legal
 *   d_votes        one uint32 per input point (that call's pair counters); may be NULL without SCVOD_OBJVIS_POOL_PAIRS
 *   d_objects      the 64-byte records the last scvod_batch_objects wrote; read only with SCVOD_OBJVIS_WITH_TRACK, and only the
 *                  `dynamic` byte of the table's objects (a SCVOD_OBJ_NO_TRACK table has 0 there)
 *   d_records      [cap_records] scvod_object_visibility, one per object in table order, or NULL: no records.  Nothing is written at or
 *                  behind cap_records; an overflow (d_records given, more objects than cap_records) is latched for the stats call and
 *                  changes no byte of d_verdict_out
 *   d_verdict_out  one byte per input point, or NULL: every member of an object with how != 0 gets the object's verdict, its UNTESTED
 *                  members included -- the occluded half goes with the half that was seen --, every other input point d_verdict[i].
 *                  d_verdict_out == d_verdict works in place.  The bytes gate scvod_map_accumulate_labelled as the per-point verdict does
 * Stream-ordered (stream NULL = the stream of the ctx's last batch call); never synchronises with the host except to grow its scratch
 * (32 bytes per SCVOD_OBJVIS_TILE input points and 8 counter words: a grow-only allocation of its own, NOT part of scvod_arena_bytes,
 * not the table's scratch), so scvod_batch_visibility -> this call -> scvod_map_accumulate_labelled on one stream needs no host read.
 * It launches and allocates nothing unless it is called and moves no other stage's state.  params NULL: the defaults.
 * SCVOD_ERR_INVALID before a device is looked for and before anything is written: NULL ctx, NULL d_verdict, an unknown flag bit,
 * reserved != 0, min_points < 1, min_tested < 1, vote_den outside 1 .. 1 << 20, vote_num outside 0 .. 1 << 20, POOL_PAIRS without
 * d_votes, WITH_TRACK without d_objects, cap_records < 0, d_votes or d_records not 4-byte aligned, d_objects not 8-byte aligned, a
 * d_verdict_out that overlaps d_verdict without being equal to it or overlaps d_votes, d_records (cap_records records) or d_objects
 * (taken to be as long as d_records: cap_records records, at least one).
 * How it runs: the sorted member list is cut into tiles of SCVOD_OBJVIS_TILE positions, whatever the objects' sizes; objects inside a
 * tile are finished by its workgroup, an object that crosses a tile edge adds integer partial counts into the 8-word accumulator of the
 * tile in which it begins, and a second launch decides it once and rewrites its pieces (csrc/scvod_objvis.hip). */
#define SCVOD_OBJVIS_POOL_PAIRS 1 /* flags bit 0: the rule reads the members' pooled pair counters, not their verdict bytes */
#define SCVOD_OBJVIS_WITH_TRACK 2 /* flags bit 1: an object whose table record has dynamic == 1 is SEEN_THROUGH whatever the vote */
#define SCVOD_OBJVIS_TILE 2048    /* member-list positions per tile */
typedef struct scvod_object_visibility_params { /* 32 bytes */
    int32_t flags;
    int32_t min_points;  /* >= 1: objects with fewer members do not vote                            */
    int32_t min_tested;  /* >= 1: nor objects with fewer members whose byte is KEEP or SEEN_THROUGH */
    int32_t min_through; /* any value                                                               */
    int32_t vote_num;    /* 0 .. 1 << 20                                                            */
    int32_t vote_den;    /* 1 .. 1 << 20                                                            */
    int32_t reserved[2]; /* 0                                                                       */
} scvod_object_visibility_params;
/* flags 0, min_points 1, min_tested 1, min_through 2, vote 1 / 2.  This project's values, NOT from real data. */
void scvod_object_visibility_params_default(scvod_object_visibility_params* p);
typedef struct scvod_object_visibility { /* 48 bytes, one per object of the table, table order */
    int32_t n_points;                                        /* == scvod_object::n_points                                         */
    int32_t n_untested, n_keep, n_seen;                      /* members by verdict byte: 2 is seen, 1 keep, every other value untested */
    int32_t sum_through, sum_agree, sum_occluded, sum_other; /* bytes 0..3 of d_votes summed over ALL members; 0 without d_votes   */
    int32_t verdict;                                         /* -1 none, SCVOD_VIS_KEEP, SCVOD_VIS_SEEN_THROUGH                    */
    int32_t how;                                             /* 0 no verdict, 1 voted, 2 forced by the table's dynamic flag        */
    int32_t reserved[2];                                     /* 0                                                                  */
} scvod_object_visibility;
int scvod_batch_object_visibility(scvod_ctx* ctx, const uint8_t* d_verdict, const uint32_t* d_votes, const void* d_objects,
                                  const scvod_object_visibility_params* params, void* d_records, int64_t cap_records,
                                  uint8_t* d_verdict_out, void* stream);
/* h_out8 = {objects of the table, objects with how == 1 (voted), objects with how == 2 (forced), objects with verdict SEEN_THROUGH,
 * members moved to SEEN_THROUGH (input byte not 2, object's verdict 2), members moved to KEEP (input byte not 1, object's verdict 1),
 * records written, 1 after an overflow} of the last call.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow,
 * with the words filled; SCVOD_ERR_STATE before the first call. */
int scvod_batch_object_visibility_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the stage holds on this ctx (0 before the first call) */
int64_t scvod_batch_object_visibility_scratch_bytes(scvod_ctx* ctx);

/* ---- the objects of a batch linked into tracks (opt-in: nothing runs or is allocated unless it is called; csrc/scvod_tracks.hip) ----
 * Reference analogue: Cluster::track_id (src/ssc.cpp:1266-1272, 1356, 1381, 1400) keeps an identity across scans, but its ids depend
 * on unordered_map iteration order and by construction never follow a moving object (a dynamic cluster is one without an overlapping
 * successor).  The rule below is this project's convention; gate and size_ratio are NOT from real data and
 * untuned.  The object table says what every cluster of every scan is; this stage says which object of the successor scan is the same
 * one.  Let A be an object of scan s and nx = next[s] >= 0:
 *   world centre  cW(A) = scvod_pose_matrix(pose_s) applied to A.center: T0*x + T1*y + T2*z + T3 per row, left to right in fp32
 *                 without contraction (the map kernel's expression)
 *   overlap (kind 1)  among A's candidates (B, count) -- B an object of scan nx, count >= 0 -- those with A.cls == 2, B.cls == 2 and
 *                 (float)count / (float)B.n_voxels >= occupancy; the largest count wins, ties to the smaller B.  This mirrors the
 *                 inheritance of ssc.cpp:1378-1385, 1408, first order
 *   gate (kind 2) only without a kind-1 proposal and without SCVOD_TRK_NO_GATE.  A needs cls == 2 (SCVOD_TRK_ANY_CLASS: any class)
 *                 and n_points >= min_points; every object B of scan nx with B.cls == A.cls, B.n_points >= min_points,
 *                 diag(A) <= size_ratio * diag(B), diag(B) <= size_ratio * diag(A) and d2 < gate * gate (the fp32 product) is
 *                 considered; diag = sqrtf((ex*ex + ey*ey) + ez*ez) of the box extents, d2 = (dx*dx + dy*dy) + dz*dz of the world
 *                 centres in fp32; the smallest d2 wins, ties to the smaller B; a NaN never qualifies
 *   acceptance    B accepts one proposer: kind 1 before kind 2, then the larger count (kind 1) or the smaller d2 (kind 2), then the
 *                 smaller A.  A refused proposer has no successor, makes no second proposal and is counted.  An accepted pair is a
 *                 link; step(B) = sqrtf(d2(A, B)), correctly rounded, for either kind
 *   tracks        the chains of links; a track is LISTED iff length >= min_length.  Tracks end at the batch's edge and at an external
 *                 successor table: nothing is carried across batches or shards
 * Every output is bit-identical from run to run and for any launch geometry. */
#define SCVOD_TRK_NO_GATE 1   /* flags bit 0: overlap links only */
#define SCVOD_TRK_ANY_CLASS 2 /* flags bit 1: the gate links objects of equal cls, not only cars */
typedef struct scvod_track_params { /* 32 bytes */
    int32_t flags;
    float occupancy;     /* negative: the ctx's params.occupancy; NaN is refused                    */
    float gate;          /* metres, > 0 and finite                                                   */
    float size_ratio;    /* >= 1                                                                     */
    int32_t min_points;  /* >= 1: smaller objects neither propose through the gate nor are proposed to */
    int32_t min_length;  /* >= 1: shorter chains are not listed                                      */
    int32_t reserved[2]; /* 0                                                                        */
} scvod_track_params;
/* flags 0, occupancy -1, gate 2.0f, size_ratio 1.5f, min_points 10, min_length 2.  This project's values, NOT from real data. */
void scvod_track_params_default(scvod_track_params* p);
typedef struct scvod_object_link { /* 32 bytes, one per object of the table, table order */
    int32_t track;    /* index in the track table, -1 when the object's track is not listed          */
    int32_t rank;     /* number of predecessors along accepted links                                  */
    int32_t pred;     /* table index of the object of the scan before that this one continues, or -1  */
    int32_t succ;     /* table index of the object that continues this one, or -1                     */
    int32_t kind;     /* how pred was linked: 0 none, 1 overlap, 2 gate                               */
    int32_t weight;   /* the overlap count for kind 1, else 0                                         */
    float step;       /* world-frame centre distance to pred, 0 without one                           */
    int32_t reserved; /* 0                                                                            */
} scvod_object_link;
typedef struct scvod_track { /* 64 bytes, one per listed track, ascending by first_object */
    int32_t first_object, last_object; /* table indices of the members with rank 0 and rank length - 1                             */
    int32_t length;                    /* members                                                                                   */
    int32_t first_scan, last_scan;     /* scvod_object::scan of the two                                                             */
    int32_t n_dynamic;                 /* members with dynamic == 1                                                                 */
    int32_t n_gate_links;              /* members with kind == 2                                                                    */
    int32_t object_begin;              /* first slot of its run in the track-object list: the member of rank r is at object_begin + r */
    float net[3];                      /* cW(last) - cW(first), per component in fp32                                               */
    float path;                        /* the members' step values summed in rank order, sequentially from 0.0f in fp32              */
    float max_step;                    /* the largest step that is not NaN; 0 without one                                            */
    int32_t reserved[3];               /* 0                                                                                         */
} scvod_track;
/* The device form works on the caller's tables, so it can be driven with crafted input.
 *   d_objects        the 64-byte records scvod_batch_objects writes; read are scan, n_points, n_voxels, box_*, center, cls, dynamic
 *   d_obj_offsets    [n_scans + 1] device array, what scvod_batch_objects writes; the true object count is d_obj_offsets[n_scans], read on
 *                    the device
 *   h_next_scan      [n_scans] or NULL (s + 1, none for the last scan), with the conventions and refusals of scvod_visibility_viewers: a
 *                    negative entry ends the chain; two scans with one successor, a scan that names itself, a ring or an entry >= n_scans
 *                    are refused
 *   h_poses          [n_scans][6] or NULL: the zero pose for every scan; staged before the call returns
 *   d_cand_begin     [objects + 1] and d_cand, int32 pairs (table index of a successor object, count): the overlap candidates of every
 *                    object.  Both may be NULL: none.  A pair whose object is not of the successor scan or whose count is negative is
 *                    skipped
 *   d_links          [cap_links] scvod_object_link or NULL.  cap_links is also the number of records of d_objects (and of entries of
 *                    d_cand_begin, less one) the caller vouches for: MORE OBJECTS THAN cap_links IS AN OVERFLOW, and then nothing is
 *                    linked and nothing is written but d_n_tracks[0] = -1
 *   d_tracks         [cap_tracks] scvod_track or NULL.  Nothing is written at or behind cap_tracks; more listed tracks than cap_tracks is
 *                    an overflow (d_n_tracks[0] = -1; the links and the track-object list are complete all the same)
 *   d_track_objects  [cap_links] int32 or NULL: the listed tracks' objects, track after track in rank order
 *   d_n_tracks       [1] int32 (device) or NULL: the listed tracks, or -1 after an overflow
 * Stream-ordered (stream NULL = the ctx's stream); never synchronises with the host except to grow its scratch (about 130 bytes per
 * record of cap_links, 56 bytes per scan, rocprim's temporary storage of a scan, 8 counter words: a grow-only allocation of its own,
 * NOT part of scvod_arena_bytes and no other stage's scratch).  It touches neither the arena nor any batch state.  params NULL: the
 * defaults.  SCVOD_ERR_INVALID before a device is looked for: NULL ctx, an unknown flag bit, a reserved word that is not 0, an
 * occupancy that is NaN, a gate that is <= 0 or not finite, size_ratio < 1 (or NaN), min_points < 1, min_length < 1, a refused successor
 * table, n_scans < 0, cap_links or cap_tracks < 0 or cap_links > 2^31 - 1, NULL d_obj_offsets, NULL d_objects with cap_links > 0, d_cand
 * without d_cand_begin, d_objects or d_cand not 8-byte aligned, any other pointer not 4-byte aligned. */
int scvod_object_tracks_device(scvod_ctx* ctx, const void* d_objects, const int32_t* d_obj_offsets, int32_t n_scans,
                               const int32_t* h_next_scan, const float* h_poses, const int32_t* d_cand_begin, const void* d_cand,
                               const scvod_track_params* params, void* d_links, int64_t cap_links, void* d_tracks, int64_t cap_tracks,
                               int32_t* d_track_objects, int32_t* d_n_tracks, void* stream);
/* The same on the table the last scvod_batch_objects (with lists) left in the ctx's scratch: d_objects are the records that call wrote
 * (cap_links of them).  The state rules are those of scvod_batch_object_shapes, and a CURRENT scvod_batch_track is needed besides: a
 * SCVOD_OBJ_NO_TRACK table is SCVOD_ERR_STATE.  The successor table is the ctx's copy from that track call (SCVOD_ERR_INVALID when the
 * rules above refuse it).  The candidates of object A are the first-order remap_name pairs of its root in the arena (what
 * scvod_batch_fetch_track reports as pair_label / pair_count), each label mapped to the object of the successor scan with that name; a
 * label that names no object of the table yields no candidate, and a successor that is an external table yields no candidates and no
 * link.  The arena, the table's scratch and scvod_arena_bytes do not change.  Stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_object_tracks(scvod_ctx* ctx, const void* d_objects, const float* h_poses, const scvod_track_params* params, void* d_links,
                              int64_t cap_links, void* d_tracks, int64_t cap_tracks, int32_t* d_track_objects, int32_t* d_n_tracks,
                              void* stream);
/* h_out8 = {objects, listed tracks found, track records written, kind-1 links, kind-2 links, proposals refused, longest listed track,
 * 1 after an overflow} of the last call of either form.  After a cap_links overflow only words 0 and 7 are filled.  Synchronises that
 * call's stream.  SCVOD_ERR_CAPACITY after an overflow, with the words filled; SCVOD_ERR_STATE before the first call. */
int scvod_object_tracks_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the stage holds on this ctx (0 before the first call) */
int64_t scvod_object_tracks_scratch_bytes(scvod_ctx* ctx);
/* Host only, no device, evaluated in double.  A track is MOVING iff sqrt(net . net) >= min_travel, STILL otherwise.  The rates are in
 * percent, NaN for a zero denominator.  SCVOD_ERR_INVALID for a NULL out, n < 0 or NULL tracks with n > 0. */
typedef struct scvod_tracks_result { /* 72 bytes */
    int64_t tracks;
    int64_t moving_tracks, moving_members, moving_members_dynamic;
    int64_t still_tracks, still_members, still_members_dynamic;
    double recall_along; /* moving_members_dynamic / (moving_members - moving_tracks): the last member of a track has no successor
                            and so can never be dynamic */
    double false_alarm;  /* still_members_dynamic / still_members */
} scvod_tracks_result;
int scvod_tracks_finish(const scvod_track* tracks, int64_t n, double min_travel, scvod_tracks_result* out);

/* ---- the tracks of a batch vote on the seen-through verdict (opt-in: nothing runs or is allocated unless it is called;
 *      csrc/scvod_trackvis.hip) ----
 * Reference analogue: none; the rule is this project's convention and its defaults are NOT from real data and
 * untuned.  Every listed track decides, and every member object takes the decision: motion along the track is a cue of its own, the
 * per-object flags pooled over the track are a vote, and an optional clear takes the stray flags of a still track back.  One
 * streaming pass rewrites the per-point verdict bytes that gate scvod_map_accumulate_labelled.  Integers and one fixed fp32
 * expression: host and device agree bit for bit, and every output is the same on every run and for any launch geometry.
 *   cW(o)      the world centre of scvod_object_tracks_device: scvod_pose_matrix(pose of objects[o].scan) applied to center, as
 *              T0*x + T1*y + T2*z + T3 per row, left to right in fp32 without contraction
 *   d2(a, b)   (dx*dx + dy*dy) + dz*dz of cW(b) - cW(a) in fp32
 * Let object o have t = links[o].track in [0, tracks), rank r = links[o].rank, L = tracks[t].length, ob = tracks[t].object_begin,
 * L >= min_length, 0 <= r < L, and let tobj be the track-object list:
 *   flagged(o)   objects[o].dynamic == 1 (not with SCVOD_TRKVIS_NO_DYNAMIC), or d_object_vis given and
 *                d_object_vis[o].verdict == SCVOD_VIS_SEEN_THROUGH.  It needs no track: it is defined for every object of the table
 *   travel2(o)   d2(cW(a), cW(b)) with a = tobj[ob + max(r - w, 0)], b = tobj[ob + min(r + w, L - 1)], w = window; window == 0: a
 *                and b are the first and the last member, tobj[ob] and tobj[ob + L - 1]
 *   moved(o)     travel2(o) >= min_travel * min_travel (the fp32 product).  A NaN never moves
 * Per track, over its L list entries m = tobj[ob + k]: n_flagged and n_moved count flagged(m) and moved(m); max_travel2 is the largest
 * travel2(m) that is not NaN.  The track VOTES THROUGH iff
 *   n_flagged >= min_flagged && (int64)n_flagged * vote_den >= (int64)vote_num * L
 * Verdict of a member, first match wins:
 *   1. moved(o), and with window == 0 also n_moved >= min_moved:   SCVOD_VIS_SEEN_THROUGH, how 2.  With window > 0 this is per
 *      member: a car that stops and goes keeps its parked phase
 *   2. the track votes through:                                    SCVOD_VIS_SEEN_THROUGH, how 1
 *   3. SCVOD_TRKVIS_CLEAR:                                         SCVOD_VIS_KEEP, how 3
 *   4. otherwise no verdict (-1, how 0)
 * An object without a listed track, or on a track below min_length (such a track is not walked: its record carries its length and
 * zeros), has no verdict.
 * Points: with o = d_point_object[i], d_verdict_out[i] = verdict(o) when o is an object of the table with a verdict, else d_verdict[i]
 * (SCVOD_VIS_UNTESTED when d_verdict is NULL).  d_verdict_out == d_verdict works in place; d_verdict_out NULL or d_point_object NULL:
 * records only.
 * Nothing read from a table is used as an index unchecked.  The latch word of the stats call collects, as bits:
 *   2  upstream overflow: d_n_tracks[0] < 0, d_obj_offsets[n_scans] (read on the device) negative or above cap_objects, more tracks than
 *      cap_tracks.  No object gets a verdict, no record is written, d_verdict_out becomes a copy of d_verdict
 *   8  a broken reference.  A track (of at least min_length) whose run [object_begin, object_begin + length) leaves [0, cap_objects) or
 *      that lists an entry outside the table is REFUSED: its record carries its length, verdict -1 and zeros, and its objects get no
 *      verdict and track -1.  An object whose links[o].track is outside [-1, tracks), or whose rank is outside [0, L) of a track that
 *      gives a verdict, gets no verdict and track -1
 *   4  a d_point_object[i] outside [-1, objects): treated as -1
 *   1  record overflow: more listed tracks than cap_track_votes or more objects than cap_object_votes (each only when its buffer is
 *      given).  Nothing is written at or behind the capacity, the records below it are complete, and NO byte of d_verdict_out changes
 * Inputs: d_objects / d_obj_offsets / d_point_object are what scvod_batch_objects wrote; d_links, d_tracks, d_track_objects and
 * d_n_tracks what scvod_object_tracks_device or scvod_batch_object_tracks wrote for the same d_objects (cap_objects records of
 * d_objects, d_links, d_track_objects and d_object_vis, cap_tracks of d_tracks: what the caller vouches for); d_object_vis the records
 * of scvod_batch_object_visibility or NULL; d_verdict any bytes, one per input point, or NULL; h_poses [n_scans][6] or NULL (the zero
 * pose), staged before the call returns.  The stage works only on these tables: it touches neither the arena nor any batch state, and
 * there are no state rules.
 * Stream-ordered (stream NULL = the ctx's stream); never synchronises with the host except to grow its scratch (22 bytes per object of
 * cap_objects -- world centre, travel2, the flag byte and the verdict byte --, 16 per track of cap_tracks, 48 per scan for the
 * matrices, 8 counter words: a grow-only allocation of its own, NOT part of scvod_arena_bytes and no other stage's scratch).
 * params NULL: the defaults.  SCVOD_ERR_INVALID before a device is looked for: NULL ctx; an unknown flag bit or a nonzero reserved
 * word; window < 0; a min_travel that is not positive and finite; min_length < 1; min_moved < 1; vote_num outside 0 .. 1 << 20 or
 * vote_den outside 1 .. 1 << 20; n_scans < 0; a negative capacity, cap_objects above 2^31 - 1 or a negative n_points; NULL
 * d_obj_offsets, d_links, d_tracks, d_track_objects or d_n_tracks; NULL d_objects with cap_objects > 0; d_verdict_out without
 * d_point_object; d_objects not 8-byte aligned, any other pointer to records or int32 not 4-byte aligned (the byte arrays may sit at
 * any address); a d_verdict_out that overlaps any input or record buffer without being equal to d_verdict. */
#define SCVOD_TRKVIS_NO_DYNAMIC 1 /* flags bit 0: the table's `dynamic` byte does not flag an object            */
#define SCVOD_TRKVIS_CLEAR      2 /* flags bit 1: members of a track that voted and did not pass become KEEP     */
typedef struct scvod_track_visibility_params { /* 40 bytes */
    int32_t flags;
    int32_t window;      /* >= 0.  0: whole-track motion (first against last member); w > 0: local motion over +-w ranks */
    float   min_travel;  /* metres, > 0 and finite */
    int32_t min_length;  /* >= 1: shorter listed tracks give no verdict */
    int32_t min_moved;   /* >= 1, read with window == 0 only, see the rule */
    int32_t min_flagged; /* any value */
    int32_t vote_num;    /* 0 .. 1 << 20 */
    int32_t vote_den;    /* 1 .. 1 << 20 */
    int32_t reserved[2]; /* 0 */
} scvod_track_visibility_params;
/* flags 0, window 0, min_travel 2.0f, min_length 2, min_moved 1, min_flagged 2, vote 1 / 2.
   This project's values, NOT from real data, untuned. */
void scvod_track_visibility_params_default(scvod_track_visibility_params* p);
typedef struct scvod_track_vote {        /* 32 bytes, one per listed track, track order */
    int32_t length, n_flagged, n_moved;
    int32_t verdict;                     /* -1 none, SCVOD_VIS_KEEP, SCVOD_VIS_SEEN_THROUGH: what members that did not move get */
    int32_t how;                         /* 0 none, 1 voted through, 3 cleared */
    float   max_travel2;                 /* largest travel2 of a member that is not NaN; 0 without one */
    int32_t reserved[2];
} scvod_track_vote;
typedef struct scvod_object_track_vote { /* 16 bytes, one per object of the table, table order */
    int32_t track;                       /* links[o].track, -1 when not listed or refused */
    int32_t verdict;                     /* -1 none, SCVOD_VIS_KEEP, SCVOD_VIS_SEEN_THROUGH */
    int32_t how;                         /* 0 none, 1 track vote, 2 motion, 3 cleared */
    float   travel2;                     /* 0 without a verdict-giving track */
} scvod_object_track_vote;
int scvod_track_visibility_device(scvod_ctx* ctx,
        const void* d_objects, const int32_t* d_obj_offsets, int32_t n_scans, const float* h_poses,
        const void* d_links, int64_t cap_objects,           /* records of d_objects / d_links the caller vouches for */
        const void* d_tracks, int64_t cap_tracks, const int32_t* d_track_objects, const int32_t* d_n_tracks,
        const void* d_object_vis,                           /* scvod_object_visibility[cap_objects] or NULL */
        const int32_t* d_point_object, const uint8_t* d_verdict, uint8_t* d_verdict_out, int64_t n_points,
        const scvod_track_visibility_params* params,
        void* d_track_votes, int64_t cap_track_votes, void* d_object_votes, int64_t cap_object_votes,
        void* stream);
/* h_out8 = {objects, listed tracks, tracks with how 1, members with how 2, members with how 3, points moved to SEEN_THROUGH (input
 * byte not 2), points moved to KEEP (input byte not 1), latch bits} of the last call; after an upstream overflow words 0 and 1 are the
 * counts as read and words 2 .. 6 are 0.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY when latch bit 1 or 2 is set, with the
 * words filled; SCVOD_ERR_STATE before the first call. */
int     scvod_track_visibility_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the stage holds on this ctx (0 before the first call) */
int64_t scvod_track_visibility_scratch_bytes(scvod_ctx* ctx);

/* ---- connected components of the map's cells, and their vote (opt-in: nothing runs or is allocated unless these are called;
 *      csrc/scvod_mapcomp.hip) ----
 * Reference analogue: none.  No program of the reference labels map cells; the conventions below are this project's (DESIGN.md
 * section 2).
 * NODES are the records of the caller's list: n 16-byte {key, val} records as scvod_map_points, scvod_map_points_labelled and
 * scvod_map_export* hand them out; only the key is read.  Every output is aligned with that list.  A record whose key is ~0 (padding)
 * or is not in the map is no node (component -1, counted).  Two records with the same key are the same cell.  A neighbouring cell is a
 * node iff the LIST holds it: a list of scvod_map_points_labelled with a select table leaves cells out of the graph (ground, say).
 * EDGES: two nodes are joined iff their cells differ by an offset in {-1, 0, 1}^3 \ {0} with |dx| + |dy| + |dz| <= 1, 2 or 3:
 * connectivity 6, 18 or 26.  Cells outside [-2^20, 2^20) on an axis do not exist; no offset carries from one axis into the next.
 *   d_component[i]  the index of record i's component, -1 for a record that is no node
 *   d_table         [cap_table] scvod_map_component, one per component
 *   d_n[0]          (device) the number of components
 * Components are numbered ascending by the SMALLEST CELL KEY they hold, so the numbering depends on the set of cells alone: not on the
 * order of the list, the table's capacity, the order of insertion or the run.  Every output is optional, but a table needs d_n.
 * Nothing is written at or behind cap_table; more components than cap_table is an overflow, latched for the stats call, and
 * d_component and d_n are complete all the same.  All reductions are integer: the outputs are bit-identical from run to run.
 * Stream-ordered against accumulate, merge and clear; reads the map's table only; never synchronises with the host except to grow its
 * scratch: 4 bytes per slot of the map, 64 bytes per record, rocprim's temporary storage of a sort of n pairs and 16 counter words, a
 * grow-only allocation of the map's own that no other stage's scratch or counter shares.
 * SCVOD_ERR_INVALID before a device is looked for: NULL map, n < 0 or n > 2^31 - 1, NULL records with n > 0, a connectivity other than
 * 6 / 18 / 26, d_records or d_table or d_n not 8-byte, d_component not 4-byte aligned, cap_table < 0, a table without d_n, outputs that
 * overlap the records or each other, a map of more than 2^30 slots.
 * How it runs: every record finds its slot and leaves its list index there (lowest wins); every node probes the half neighbourhood
 * (3 / 9 / 13 cells) and unites itself with the nodes it finds in a lock-free union-find over list indices (path halving, the larger
 * root hooked under the smaller by compare-and-swap; no grid barrier, no waiting); a flatten pass; count, smallest key and box are
 * reduced per root through an LDS table per workgroup; the roots are sorted by smallest key and the rank becomes the index. */
typedef struct scvod_map_component { /* 48 bytes */
    uint64_t key;                     /* smallest cell key of the component                */
    int32_t n_records;                /* its records, duplicates included                  */
    int32_t first_record;             /* lowest list index among them                      */
    int32_t cell_min[3], cell_max[3]; /* signed cell coordinates, inclusive                */
    int32_t reserved[2];              /* 0                                                 */
} scvod_map_component;
int scvod_map_components(scvod_map* map, const void* d_records, int64_t n, int32_t connectivity, int32_t* d_component, void* d_table,
                         int64_t cap_table, int64_t* d_n, void* stream);
/* h_out8 = {records, nodes, padding records, records whose key is absent, duplicate records, components, table records written,
 * 1 after an overflow} of the last call.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an overflow, with the words
 * filled; SCVOD_ERR_STATE before the first call. */
int scvod_map_components_stats(scvod_map* map, int64_t* h_out8);
/* bytes of device scratch the labelling holds on this map (0 before the first call) */
int64_t scvod_map_components_scratch_bytes(const scvod_map* map);

/* The components vote on the seen-through verdict: the rule of scvod_batch_object_visibility, restated for components.  The rule and
 * the defaults are this project's convention and NOT from real data.
 *   d_component    [n] what scvod_map_components wrote for the same list; d_n (device) its component count
 *   d_verdict      [n] one byte per record, what scvod_cloud_visibility_device wrote for the same points; any bytes are legal
 *   d_votes        [n][4] uint16 {n_through, n_agree, n_occluded, n_empty} of that call, or NULL without SCVOD_CMPVIS_POOL_PAIRS
 * Per component, over its members (the records with its index): n_seen / n_keep / n_untested = members whose byte is 2 / 1 / anything
 * else; the four counters summed over ALL members in int64.  With t = n_seen, a = n_keep (SCVOD_CMPVIS_POOL_PAIRS: t = sum_through,
 * a = sum_agree) a component VOTES iff
 *   n_records >= min_cells && (max_cells == 0 || n_records <= max_cells) && n_keep + n_seen >= min_tested
 * and its verdict is SCVOD_VIS_SEEN_THROUGH iff
 *   t >= min_through && t * vote_den >= vote_num * (t + a)          (int64; the sums stay below 2^47, the products below 2^60)
 * and SCVOD_VIS_KEEP otherwise (how = 1).  Every other component has verdict -1, how 0.
 *   d_verdict_out  [n] or NULL: every member of a component that voted takes its verdict, UNTESTED members included; a record keeps
 *                  its byte if its component is -1, did not vote, or has an index at or beyond cap_components.
 *                  d_verdict_out == d_verdict works in place
 *   d_records      [cap_records] scvod_component_visibility, one per component, or NULL.  Nothing is written at or behind cap_records;
 *                  more components (below cap_components) than cap_records is an overflow, latched for the stats call
 * d_n is read on the device: scvod_cloud_visibility_device -> scvod_map_components -> this call -> scvod_map_accumulate_labelled on one
 * stream needs no host read.  Stream-ordered; never synchronises except to grow its scratch (48 bytes per component up to
 * min(cap_components, n), 8 counter words: a grow-only allocation of the map's own).  params NULL: the defaults.
 * SCVOD_ERR_INVALID before a device is looked for: NULL map, n < 0 or n > 2^31 - 1, NULL d_n, NULL d_component or d_verdict with n > 0,
 * cap_components < 0, cap_records < 0, an unknown flag bit, reserved != 0, min_cells < 1, max_cells < 0, min_tested < 1, vote_den
 * outside 1 .. 4096, vote_num outside 0 .. 4096, POOL_PAIRS without d_votes, d_component not 4-byte, d_n or d_votes or d_records not
 * 8-byte aligned, a d_verdict_out that overlaps d_verdict without being equal to it or overlaps another argument. */
#define SCVOD_CMPVIS_POOL_PAIRS 1 /* flags bit 0: the rule reads the members' pooled pair counters, not their verdict bytes */
typedef struct scvod_component_visibility_params { /* 32 bytes */
    int32_t flags;
    int32_t min_cells;   /* >= 1: components with fewer records do not vote                             */
    int32_t max_cells;   /* >= 0: nor components with more; 0: no upper limit                           */
    int32_t min_tested;  /* >= 1: nor components with fewer members whose byte is KEEP or SEEN_THROUGH  */
    int32_t min_through; /* any value                                                                   */
    int32_t vote_num;    /* 0 .. 4096                                                                   */
    int32_t vote_den;    /* 1 .. 4096                                                                   */
    int32_t reserved;    /* 0                                                                           */
} scvod_component_visibility_params;
/* flags 0, min_cells 1, max_cells 0, min_tested 1, min_through 2, vote 1 / 2.  This project's values, NOT from real data. */
void scvod_component_visibility_params_default(scvod_component_visibility_params* p);
typedef struct scvod_component_visibility { /* 64 bytes, one per component, component order */
    int32_t n_records;                                       /* members in the list                                           */
    int32_t n_untested, n_keep, n_seen;                      /* members by verdict byte: 2 is seen, 1 keep, every other untested */
    int64_t sum_through, sum_agree, sum_occluded, sum_empty; /* the four counters of d_votes over ALL members; 0 without d_votes */
    int32_t verdict;                                         /* -1 none, SCVOD_VIS_KEEP, SCVOD_VIS_SEEN_THROUGH               */
    int32_t how;                                             /* 0 no verdict, 1 voted                                         */
    int32_t reserved[2];                                     /* 0                                                             */
} scvod_component_visibility;
int scvod_map_component_visibility(scvod_map* map, const int32_t* d_component, int64_t n, const int64_t* d_n, int64_t cap_components,
                                   const uint8_t* d_verdict, const uint16_t* d_votes, const scvod_component_visibility_params* params,
                                   void* d_records, int64_t cap_records, uint8_t* d_verdict_out, void* stream);
/* h_out8 = {components (d_n), voted, SEEN_THROUGH, members moved to SEEN_THROUGH, members moved to KEEP, records written, components at
 * or beyond cap_components, 1 after an overflow} of the last call.  Synchronises that call's stream.  SCVOD_ERR_CAPACITY after an
 * overflow, with the words filled; SCVOD_ERR_STATE before the first call. */
int scvod_map_component_visibility_stats(scvod_map* map, int64_t* h_out8);

/* ---- refining scan poses against the static map or a cloud (opt-in: nothing runs or is allocated unless these are called;
 *      csrc/scvod_register.hip) ----
 * Reference analogue: none (its src/gicp.cpp concatenates PCD files).  The definition is this project's.
 * Every other stage takes the caller's poses as exact; this one improves them by Gauss-Newton on nearest-point correspondences, all
 * iterations enqueued on the stream without a host read in between.  The step is defined once, in csrc/scvod_math.h (reg_*):
 *   T_s        the running pose of scan s, a row-major 3x4 in fp64 on the device (d_pose_out); initially the fp32 matrix
 *              scvod_pose_matrix(h_poses + 6 s) widened (h_poses NULL: the zero pose), so iteration 0 sees the points scvod_map_query sees
 *   moving     a source point p (packed float4 in the sensor frame; w is not read) goes to T0*x + T1*y + T2*z + T3 per row, left to
 *              right in fp32, with the fp32 rounding of T_s
 *   skipped    and counted, each in its own counter: a NaN coordinate; (x*x + y*y) + z*z > max_range * max_range in fp32; a label
 *              byte whose use256 entry is 0; no correspondence; (plane mode) a target normal that is not finite or shorter than 1e-6
 *   q          the target's nearest point under the target's own rule (below) at squared fp32 distance d < max_dist * max_dist
 *   residual   for the right perturbation T <- T * exp(xi), xi = (omega, v).  SCVOD_REG_POINT: three rows r = p - R^T (q - t),
 *              J = [ -[p]x , I ].  SCVOD_REG_PLANE: one row e = n_l . r with n_l = R^T (n / |n|), J = [ (p x n_l)^T , n_l^T ]
 *   sums       per scan the 21 + 6 + 1 entries of J^T J (upper triangle), J^T r and sum r^2: every term in fp64 from the fp32 inputs,
 *              times 2^20, rounded to nearest and added as int64 -- the sums do not depend on the order of the points, the launch
 *              geometry or the run.  No sum can overflow with max_range <= 256, max_dist <= 256 and at most 2^24 points per scan;
 *              a larger or infinite max_range is accepted and leaves that bound to the caller (points * range^2 < 2^41)
 *   solve      fp64: H = sums / 2^20, H_ii += lambda * H_ii, LDL^T.  DEGENERATE (the pose is kept) with fewer than min_corr
 *              correspondences, a pivot not above pivot_eps * max H_ii, or a step that is not finite
 *   update     the unit quaternion of (1, omega / 2) as a rotation dR (a Cayley step): R <- R dR, t <- R v + t; only + - * / sqrt
 *   CONVERGED  |omega| < eps_rot and |v| < eps_trans for the step just applied.  A converged or degenerate scan is latched in its
 *              record: later iterations return at once for it and its pose does not change again
 * The rotation stays as orthonormal as the initial fp32 matrix is (about 1e-7): each dR is orthonormal to a few ulp of fp64.
 * Device and host agree bit for bit (tests/helpers/register_ref.cpp runs the same functions on the CPU).
 * scvod_pose_from_matrix turns a refined matrix (narrowed to float) into the {x, y, z, roll, pitch, yaw} the other calls take; that
 * round trip goes through fp32 Euler angles and is NOT bit-exact. */
#define SCVOD_REG_POINT 0 /* mode: point-to-point */
#define SCVOD_REG_PLANE 1 /* mode: point-to-plane (a cloud target with normals only) */
#define SCVOD_REG_MAX_ITERATIONS 0 /* status: max_iterations ran without convergence */
#define SCVOD_REG_CONVERGED 1
#define SCVOD_REG_DEGENERATE 2
typedef struct scvod_register_params {
    int32_t max_iterations; /* 1 .. 64                                                                        */
    int32_t min_corr;       /* >= 6: fewer correspondences make the scan DEGENERATE                           */
    int32_t mode;           /* SCVOD_REG_POINT / SCVOD_REG_PLANE                                              */
    int32_t reserved;       /* 0                                                                              */
    float max_dist;         /* > 0, <= 256 (map target: <= 0.99f * leaf)                                      */
    float max_range;        /* > 0; +inf: no range gate                                                       */
    double eps_rot;         /* >= 0, radians                                                                  */
    double eps_trans;       /* >= 0, metres                                                                   */
    double lambda;          /* >= 0: Levenberg damping of the diagonal                                        */
    double pivot_eps;       /* >= 0                                                                           */
    const uint8_t* use256;  /* [256] host bytes over the label byte, read before the call returns; NULL: all  */
} scvod_register_params;
/* max_iterations 10, min_corr 30, POINT, max_dist 0.19, max_range 80, eps_rot 1e-6, eps_trans 1e-5, lambda 0, pivot_eps 1e-9, use256
 * NULL.  This project's values, untuned and NOT from real data. */
void scvod_register_params_default(scvod_register_params* p);
/* What the three calls below refuse before a device is touched, as a host-only function: SCVOD_ERR_INVALID for max_iterations outside
 * 1 .. 64, min_corr < 6, an unknown mode, reserved != 0, max_dist not in (0, 256], max_range not > 0, a negative or NaN eps_rot,
 * eps_trans, lambda or pivot_eps; with leaf > 0 (a map target): max_dist > 0.99f * leaf or plane mode; with leaf == 0 (a cloud
 * target): plane mode without normals (has_normals == 0); a d_src_xyzi that is not 16-byte aligned.  params NULL: the defaults. */
int scvod_register_check(const scvod_register_params* params, float leaf, int32_t has_normals, const void* d_src_xyzi);
typedef struct scvod_register_record { /* 64 bytes, one per scan */
    int32_t status;       /* SCVOD_REG_*                                                                     */
    int32_t iterations;   /* accumulate + solve rounds this scan took part in                                */
    int64_t n_corr;       /* correspondences of the last accumulation                                        */
    double sum_r2;        /* its sum of squared residuals (the int64 sum / 2^20)                             */
    double last_omega;    /* |omega| and |v| of the last step (0 for a DEGENERATE round)                     */
    double last_v;
    int32_t skip_nan, skip_range, skip_label, skip_no_corr, skip_normal; /* of the last accumulation         */
    int32_t reserved;     /* 0                                                                               */
} scvod_register_record;
/* Against the static map (both kinds), point-to-point.  The candidate rule is the query's: the nearest decoded representative among
 * the own cell and the 26 around it (csrc/scvod_mapprobe.h, shared with the query and the filter), ties to the smaller key, the
 * select table honoured (labelled maps only) -- a scan's correspondences of iteration 0 are the points whose d_nn_key != ~0 in
 * scvod_map_query with the same poses, radius = max_dist and select table.  Only reads the table: no record, no counter and no scratch
 * of the accumulate, query, filter or component calls moves.
 *   d_xyzi [h_scan_offsets[n_scans]][4], 16-byte aligned; d_labels one byte per point or NULL (then use256 is not read)
 *   d_pose_out [n_scans][12] doubles, 8-byte aligned; d_records [n_scans] scvod_register_record, 8-byte aligned; both required
 * Stream-ordered: max_iterations rounds of {k_reg_accumulate, k_reg_solve} are enqueued and the call returns; it synchronises only to
 * grow its scratch (grow-only, the map's own, a few hundred bytes per scan: scvod_map_register_scratch_bytes reports it), for poses or
 * offsets that differ from the previous call's, and behind a call in flight on another stream.  params NULL: the defaults. */
int scvod_map_register(scvod_map* map, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                       const uint8_t* d_labels, const scvod_register_params* params, const uint8_t* h_select256, double* d_pose_out,
                       void* d_records, void* stream);
/* The same for the input cloud of the ctx's last batch, obtained as scvod_batch_map_query obtains it.  d_labels is typically the output
 * of scvod_batch_point_labels with a use256 that leaves out SCVOD_PT_DYNAMIC, so that moving objects do not pull the pose.
 * SCVOD_ERR_STATE without a processed batch; stream NULL = the stream of the ctx's last batch call. */
int scvod_batch_map_register(scvod_ctx* ctx, scvod_map* map, const float* h_poses, const uint8_t* d_labels, const scvod_register_params* params,
                             const uint8_t* h_select256, double* d_pose_out, void* d_records, void* stream);
/* h_out8 = {scans, CONVERGED, MAX_ITERATIONS, DEGENERATE, correspondences of the last accumulations, iterations summed over the scans,
 * points skipped in the last accumulations, source points} of the last call.  Synchronises that call's stream.  SCVOD_ERR_STATE before
 * the first call. */
int scvod_map_register_stats(scvod_map* map, int64_t* h_out8);
int64_t scvod_map_register_scratch_bytes(const scvod_map* map);
/* Against a cloud: d_tgt_xyz [n_tgt][3] packed floats (finite) in the frame the poses map into, d_tgt_normals [n_tgt][3] or NULL (plane
 * mode requires them).  The grid is the shared one of the nearest-neighbour stages (csrc/scvod_grid.h) as scvod_nn_radius_search sizes
 * it: cell edge max(max_dist, 0.2f), widened to max_dist / 0.98f when max_dist * max_dist > (0.99f * edge)^2 so that the 27 cells hold
 * every point within max_dist; origin 0; the 27-cell probe, ties to the lowest index.  It is built once per call and reused by every
 * iteration.  Scratch: grow-only, the ctx's own (scvod_register_scratch_bytes); scvod_arena_bytes does not move.  n_tgt == 0 is legal
 * (every scan DEGENERATE).  Otherwise as scvod_map_register; stream NULL = the ctx's stream. */
int scvod_register_device(scvod_ctx* ctx, const void* d_src_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                          const uint8_t* d_labels, const float* d_tgt_xyz, const float* d_tgt_normals, int32_t n_tgt,
                          const scvod_register_params* params, double* d_pose_out, void* d_records, void* stream);
int scvod_register_stats(scvod_ctx* ctx, int64_t* h_out8);
int64_t scvod_register_scratch_bytes(scvod_ctx* ctx);

/* ---- surface normals and curvature of a cloud or of the static map's points (opt-in: nothing runs or is allocated unless these are
 *      called; csrc/scvod_normals.hip) ----
 * Reference analogue: none for an arbitrary cloud (SSC::intensityCalibrationByCurvature runs pcl::NormalEstimationOMP with the k nearest
 * points of one scan; that stage is scvod_set_intensity_calibration).  The definition is this project's; it is
 * what SCVOD_REG_PLANE of scvod_register_device needs of its target.  Defined once, in csrc/scvod_math.h (nrm_*, normal_finish):
 *   neighbours  of a query q: every cloud point p with fp32 d = (ex*ex + ey*ey) + ez*ez < radius * radius, e = p - q one fp32
 *               subtraction per component.  q itself is a neighbour when it is a point of the cloud (d == 0).  Radius based, not kNN:
 *               the set does not depend on any order
 *   left out    and counted: a cloud point with a NaN or infinite coordinate or |c| > 1e6 is never a neighbour; such a query gets NaN
 *   sums        ten int64 words per query: the count k, the sums of e_a (x, y, z) and of e_a * e_b (xx, xy, xz, yy, yz, zz).  A term
 *               is the fp64 product of the fp32 offsets (exact), times 2^30, rounded to nearest (ties to even): the sums do not depend
 *               on the order of the points, the launch geometry or the run.  No sum can overflow with radius <= 4 and at most 2^28
 *               cloud points; anything beyond is refused
 *   finish      fp64: m_a = S_a / 2^30 / k, c_ab = S_ab / 2^30 / k - m_a * m_b; narrowed to float; the normal is the eigenvector of
 *               the smallest eigenvalue by the solver of the intensity calibration and the region growing (one eigen specification),
 *               the curvature |eigenvalue / ((c_xx + c_yy) + c_zz)|, 0 for a zero trace.  k < min_neighbours: NaN normal and
 *               curvature.  A zero covariance gives the solver's NaN normal; plane-mode registration skips and counts such normals
 *   orientation optional: queries h_seg_offsets[s] .. h_seg_offsets[s + 1] see the viewpoint h_viewpoints[3 s ..]; a normal is negated
 *               iff fp32 ((vx - qx) * nx + (vy - qy) * ny) + (vz - qz) * nz < 0 (pcl::flipNormalTowardsViewpoint).  n_segments == 0:
 *               the solver's sign stays (the plane residual of the registration does not depend on it)
 * The grid is the shared one of the nearest-neighbour stages (csrc/scvod_grid.h) as scvod_nn_radius_search sizes it: cell edge
 * max(radius, 0.2f), widened to radius / 0.98f when radius * radius > (0.99f * edge)^2 so that the 27 cells hold every point within
 * the radius; origin 0.  As for that search, the neighbourhood is exactly the one defined above while |c| <= 25000 * edge on every axis;
 * beyond it (up to 1e6) a neighbour near the radius may be missed.  Every point counts once, however many of the 27 cells share a
 * bucket.  Device and host agree bit for bit (tests/helpers/normals_ref.cpp runs the same functions over an exhaustive loop).
 * One call sees one cloud: a batch of scans in their sensor frames needs the world-frame export (scvod_batch_export_points with poses)
 * or one call per scan.  Per-segment neighbourhoods are out of scope; the segments only choose the viewpoint. */
typedef struct scvod_normal_params {
    float radius;           /* > 0, <= 4                                                                      */
    int32_t min_neighbours; /* >= 3: a query with fewer neighbours (itself included) gets NaN                 */
    int32_t flags;          /* 0                                                                              */
    int32_t reserved;       /* 0                                                                              */
} scvod_normal_params;
/* radius 0.5, min_neighbours 5.  This project's values, untuned and NOT from real data. */
void scvod_normal_params_default(scvod_normal_params* p);
/* What the calls below refuse before a device is touched, as a host-only function: SCVOD_ERR_INVALID for a radius not in (0, 4],
 * min_neighbours < 3, flags or reserved != 0, a cloud_stride other than 3 or 4, a query_stride other than 3, 4 or 0 (0: the self
 * form), n_cloud < 0 or > 2^28, n_query < 0 or > 2^31 - 1, n_segments < 0, offsets or viewpoints with n_segments == 0, viewpoints
 * without offsets or offsets without viewpoints, offsets that do not start at 0, decrease or do not end at n_query.  params NULL: the
 * defaults. */
int scvod_normals_check(const scvod_normal_params* params, int32_t cloud_stride, int64_t n_cloud, int32_t query_stride, int64_t n_query,
                        const int32_t* h_seg_offsets, const float* h_viewpoints, int32_t n_segments);
/* d_cloud [n_cloud][cloud_stride] floats (xyz first; stride 3 or 4), d_query [n_query][query_stride] or NULL: the queries are the
 * cloud (then n_query == n_cloud and query_stride is not read).  d_normals [n_query][3] packed floats -- exactly what
 * scvod_register_device takes as d_tgt_normals; d_curvature [n_query], d_count [n_query] int32 (k) and d_sums [n_query][10] int64
 * are optional (NULL).  A query that is not finite gets NaN, k 0 and zero sums.  n_cloud == 0 or n_query == 0 is legal.
 * Stream-ordered (stream NULL = the ctx's stream): k_nrm_keep, the grid build and k_nrm_accumulate are enqueued and the call returns;
 * the host arrays are copied before it does.  It synchronises only to grow its scratch (grow-only, the ctx's own:
 * scvod_normals_scratch_bytes; the grid's work area, a keep byte per cloud point, eight counter words, the segment tables --
 * scvod_arena_bytes and every other stage's scratch do not move).  A call on another stream of the same ctx is ordered behind the
 * last one on the device (an event), not on the host: the calls of one ctx share the scratch and run one after the other. */
int scvod_normals_device(scvod_ctx* ctx, const float* d_cloud, int32_t cloud_stride, int32_t n_cloud, const float* d_query, int32_t query_stride,
                         int32_t n_query, const int32_t* h_seg_offsets, const float* h_viewpoints, int32_t n_segments,
                         const scvod_normal_params* params, float* d_normals, float* d_curvature, int32_t* d_count, int64_t* d_sums, void* stream);
/* h_out8 = {queries, finite normals, queries below min_neighbours, queries that are not finite, cloud points left out, largest k, sum
 * of k, 0} of the last call (the map form included).  Synchronises that call's stream.  SCVOD_ERR_STATE before the first call. */
int scvod_normals_stats(scvod_ctx* ctx, int64_t* h_out8);
/* bytes of device scratch the normals hold on this ctx (0 before the first call) */
int64_t scvod_normals_scratch_bytes(scvod_ctx* ctx);
/* The static map as points with their normals: scvod_map_points (a plain map) or scvod_map_points_labelled (a labelled map; only
 * there h_select256 and d_labels are legal) into d_xyzi [cap][4], 16-byte aligned, followed by the self form above with stride 4 into
 * d_normals [cap][3] and d_curvature [cap] (optional).  Row i of every output is the same cell; the order is unspecified.  It
 * synchronises `stream` and reports *n_out and SCVOD_ERR_CAPACITY exactly as those two calls do (nothing is written at or behind cap,
 * and no normal at all); the normals are then stream-ordered behind the points (stream NULL = the ctx's stream).  Only the export
 * counters of the map move, as in those calls; the scratch is the ctx's (scvod_normals_scratch_bytes).  Errors are reported on the
 * ctx (scvod_last_error).  The packed [n][3] target scvod_register_device wants is a copy of the first three columns of d_xyzi.
 * scvod_map_register keeps refusing plane mode: the map's normals go through scvod_register_device. */
int scvod_map_points_normals(scvod_ctx* ctx, scvod_map* map, const scvod_normal_params* params, const uint8_t* h_select256, void* d_xyzi,
                             uint8_t* d_labels, float* d_normals, float* d_curvature, int64_t cap, int64_t* n_out, void* stream);
/* Development switch behind profiles/normals_cost.txt and the tests, never needed for a result: the low two bits choose the arm of the
 * self form (0: the default; 1: a thread per query in the caller's order; 2: a thread per grid entry, so that the lanes of a wave share
 * buckets), bit 2 launches workgroups of 64 threads in place of 256.  The outputs are identical. */
int scvod_set_normals_variant(scvod_ctx* ctx, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* SCVOD_H_ */
