// scvod_kernels.h -- launch interface between the C-ABI layer (scvod_capi.hip) and the
// gfx950 kernels (scvod_kernels.hip).  All pointers are device pointers.
#ifndef SCVOD_KERNELS_H_
#define SCVOD_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/scvod.h"
#include "scvod_math.h"

namespace scvod {

constexpr int kMaxPatches = SCVOD_MAX_PATCHES;
constexpr int kMaxBuckets = 1024;
constexpr int kVgLutBins = 16384;
constexpr int kIrrListCap = 256;  // points of a scan with an index triple outside the grid that k_emit lists (Arena::irr_list)
// marks per INPUT point for the static map, which streams the input in order: whether Patchwork kept a point at all follows
// from its patch id (pid) and that patch's population; k_tk_dyn marks the members of dynamic clusters; the two list marks are
// only written when a caller asks for a map without the ground or without the range/FOV rejects
constexpr uint8_t kMapDynamic = 1, kMapGround = 2, kMapRejected = 4, kMapCar = 8;  // (kMapCar: member of a `car` cluster, set by the clustering:
                                                                                    //  the only points a tracking result can take out of the map)

struct Xyz {
    float x, y, z;
};

struct DevParams {
    BinParams bin;
    CzmParams czm;
    KeepFast keep;       // shortcut of the range / FOV verdict (scvod_math.h::keep_of_point)
    BinFast binfast;     // guarded estimate of a transformed point's voxel index (scvod_math.h::voxel_idx_fast)
    int64_t key_off;     // added to voxel_idx before bucketing (R*S + S + 1)
    int32_t vb_shift;    // bucket = clamp((voxel_idx + key_off) >> vb_shift, 0, n_buckets-1)
    int32_t n_buckets;
    int32_t n_patches;
    float max_z, min_z, car_square;  // recognise thresholds (utility.h:294-298)
    int32_t to_be_class;             // utility.h:306
};

// per-patch record produced by the patch kernel, consumed by the emission kernels
struct PatchRec {
    int32_t n;       // points in the patch (pc2czm)
    int32_t n_g;     // size of the ground part after the last iteration
    int32_t status;  // 0 skipped, 1 kept, 2 rejected (tilt), 3 rejected (elevation+flatness)
    int32_t a_g;     // points of the ground part that pass the range/FOV filter of makeApriVec
    int32_t a_ng;    // same for the non-ground part
};

// Device arena of one batch.  Per-point arrays are indexed by scan_off[s] + local index;
// per-scan arrays by s * stride.
// board of k_cc_scan's shared exact re-clustering (scvod_k_cluster.inc, cc_help_loop): header [0] slots taken, [1] scans past their exact phase;
// per slot: [0,1] claim word (round << 32 | next chunk), [2] chunks done by helpers, [3] listed nodes, [4] chunks per round, [6..17] six table pointers of the rounds, [26..35] five more for the passes after them, [18..25] development clocks
constexpr int kCcHelpSlots = 256, kCcHelpHdr = 32, kCcHelpSlotWords = 64;  // (a slot = two 128-byte lines of its own)
constexpr size_t kCcHelpWords = kCcHelpHdr + (size_t)kCcHelpSlots * kCcHelpSlotWords;
constexpr int kCcExactBlocks = 256, kCcExactLeaders = 160;  // grid of k_cc_exact; blocks that lead a listed scan at most (the others help)
struct Arena {
    // inputs
    const float4* pts;
    const int32_t* scan_off;  // [B+1]
    int32_t n_scans;
    int32_t max_scan_pts;
    int64_t total_pts;
    // patchwork
    int16_t* pid;             // [N] patch id or -1
    uint64_t* keys;           // [N] (sortable z << 32 | local idx), patch-major per scan
    uint32_t* seg;            // [N] per patch: [ground part -> | <- non-ground part (stored back to front)], bit31 = passes bin filter
                              //   (input of k_emit_lists while the three index lists of a lean batch are pending)
    uint32_t* ln_scratch;     // [N] 4 bytes per input point for the class tables of the max_name pass in arena scratch: seg once the three
                              //   lists are written, ground_idx while they are pending (k_emit_lists rewrites it wholly): one of the two
                              //   stays intact.  Set by the ctx before every clustering.
    Xyz* sorted_xyz;          // [N] per patch: points in (z, idx) order, packed 12-byte xyz
    uint32_t* sorted_idx;     // [N] same order: input index | (passes the range/FOV test) << 31
    uint32_t* zkey;           // [N] sortable z key per input point (k_pw_classify -> k_pw_scatter); then, lean emission: packed index triple of
                              //   the kept points at the position of their seg word (arrange pass -> k_emit<true>); then scratch of the max_name pass
    float* fit_thd;           // [B][kMaxPatches] th_dist_d_ of the last plane fit
    int4* order;              // [B * kMaxPatches] live patches by descending size class: {scan*1024+patch, n, scan base, patch offset}
    int32_t* order_hist;      // [64]
    int32_t* order_cursor;    // [64]
    int32_t* order_off;       // [65]  ([64] = number of live patches)
    int32_t* patch_count;     // [B][kMaxPatches]
    int32_t* patch_cursor;    // [B][kMaxPatches]
    int32_t* patch_off;       // [B][kMaxPatches+1]
    PatchRec* patch_rec;      // [B][kMaxPatches]
    scvod_patch_plane* planes;  // [B][kMaxPatches]
    int32_t* emit_off;        // [B][kMaxPatches][4]  ground / nonground / apri / rejected
    // outputs of the Patchwork + binning stage
    uint8_t* cls;             // [N] filled per scan on request (scvod_batch_fetch / per-scan API), see k_cls_from_lists
    int32_t* ground_idx;      // [N]  (the three lists: ground_idx, nonground_idx, rejected_src -- written by k_emit<false>; a lean batch
    int32_t* nonground_idx;   // [N]   leaves them to k_emit_lists, on demand)
    scvod_apri* apri;         // [N]
    int32_t* apri_src;        // [N]
    int32_t* apri_key;        // [N] PointAPRI::voxel_idx, compact copy for the voxel stage
    float* apri_int;          // [N] PointAPRI::intensity, compact copy for the voxel stage (a lean emission leaves it to k_apri_intensity, on demand)
    int32_t* apri_idx3;       // [N] PointAPRI::{range,sector,azimuth}_idx packed 11+11+10 bits (clustering)
    int32_t* rejected_src;    // [N]
    int32_t* counts;          // [B][8]
    int32_t* scan_irr;        // [B] != 0: the scan holds an index triple outside the grid (set by the binning kernels; only orders the clustering)
    int32_t* irr_list;        // [B][kIrrListCap + 1] [0] = how many points of the scan have an index triple outside the grid (-1: not listed by the
                              //   kernel that binned the batch), then their apri indices: k_emit -> scvod_lastname.hip
    int32_t* cc_perm;         // [B] order in which k_cc_scan takes the scans: the irregular ones (the long-running workgroups) first
    // voxel stage
    int32_t* vb_count;        // [B][kMaxBuckets]
    int32_t* vb_off;          // [B][kMaxBuckets+1]
    int32_t* vb_nvox;         // [B][kMaxBuckets]
    int32_t* vox_off;         // [B][kMaxBuckets+1]
    int4* vorder;             // [B * kMaxBuckets] non-empty buckets by descending size class (same item layout)
    int32_t* vorder_hist;     // [64]
    int32_t* vorder_cursor;   // [64]
    int32_t* vorder_off;      // [65]
    uint64_t* vkeys;          // [N] (biased voxel key << 32 | apri idx), bucket-major per scan; or 32-bit keys (vx_k32)
    int32_t vx_k32;           // 1: the voxel stage of this batch sorts 32-bit keys: (key - bucket's first key) << vx_idx_bits | apri idx
                              //    (range/FOV-filtered keys only: every key lies inside its bucket's range; vb_shift + vx_idx_bits <= 32)
    int32_t vx_idx_bits;      // bits of an apri index inside one scan of this batch
    int32_t* tmp_vox_key;     // [N] per-bucket voxel records before compaction
    int32_t* tmp_vox_begin;   // [N]
    float* tmp_vox_av;        // [N]
    float* tmp_vox_cov;       // [N]
    int32_t* vox_key;         // [N]
    int32_t* vox_pt_begin;    // [N + B]  (n_vox + 1 entries per scan, base scan_off[s] + s)
    int32_t* vox_pts;         // [N]
    float* vox_av;            // [N]
    float* vox_cov;           // [N]
    // clustering (connected components of occupied voxels)
    int32_t cc_exact_max;     // generic clustering variant: nodes of components with irregular runs that are re-clustered exactly
                              //   (default 4096; scvod_set_cluster_exact(ctx, 1 or 2) lifts it to "any")
    int32_t cc_plain_rule;    // 1: irregular runs that the cells around them settle are left as found (cc_run_is_plain); 0: every one is re-clustered
    int32_t* cc_stats;        // [8] per clustering call: [4] irregular runs settled by the rule, [5] the others; [0..3] scans that kept "everything found is joined" for a component, nodes of
                              //   those components (an upper bound from a sample when they are not even listed), 0, scans of the generic variant
                              //   whose z-planes are too large for the windowed search (forest in HBM)
    int32_t* cc_again;        // [1 + B] scans k_cc_scan hands over to k_cc_exact: [0] how many, then the scans; [0] cleared per launch
    int32_t* cc_help;         // [kCcHelpWords] board of the exact re-clustering rounds that leaders share with helper blocks (scvod_k_cluster.inc: cc_help_loop); cleared per launch
    int32_t cc_help_blocks;   // > 0: the blocks of k_cc_exact that lead no scan help (set per launch by launch_cluster)
    int32_t cc_help_blocks_wanted;  // what the ctx asks for (0 = leaders always work alone: tests / A-B runs)
    int32_t* cc_parent;       // [N] union-find forest over apri indices (scan-local)
    uint8_t* cc_touched;      // [N] per voxel slot: appeared in a neighbourhood
    int32_t* pt_voxel;        // [N] voxel slot of every apri point
    int32_t* pt_cluster;      // [N] canonical cluster name = smallest apri index of the component
    uint32_t* cl_bbox;        // [7N] clustering scratch: bounding-box records of the scans that do not fit the LDS
    int32_t* cl_count;        // [N] per cluster root: number of points
    uint8_t* pt_type;         // [N] per apri point: 0 erased, 1 other, 2 car
    // the cluster that still carries Frame::max_name as ssc.cpp:354 stores it (scvod_lastname.hip)
    int32_t* cc_last;         // [B][4] {canonical name or -1, lowest voxel slot whose first point belongs to it or -1,
                              //         status: 0 exact, 1 a replay did not fit the LDS, 2 too many index triples outside the grid, events replayed}
    int32_t* cc_redo;         // 4 x [B + 1] scans listed by the triage for the pass with the small / mid / large tables, [B] = how many
    int32_t* ln_state;        // [B][kLnStateWords] what the triage leaves a scan's follow-up pass: the set of classes, the irregular points, the class table
    int32_t* ln_prof;         // [B][8] phase clocks (10 ns ticks) and counts of the last pass over a scan: tools/lastname_lat.py
    int32_t* ln_prof2;        // [B][8] the largest class walked: nodes, Jacobi rounds, clocks of build / rounds / openers / partition / walk, events
    int32_t* ln_stats;        // [4] per clustering call: scans with status 1, with status 2, 0, 0
    // sequence differencing on the device (scvod_batch_track, scvod_track.hip)
    int4* vox_track;          // [N] per voxel: {key, label = cluster root of its points or -1, |occupy_voxels| of that
                              //     cluster, its type}: the table the probe of the PREVIOUS scan runs against; also the
                              //     boundary message between sequence shards (scvod_batch_export_table)
    int32_t* vox_rep;         // [N] per voxel: lowest voxel slot of the scan that carries the same label (-1: unlabelled): the
                              //     label's id in the sequential tracking chain (scvod_chain.hip)
    int32_t* tk_crep;         // [N] per scan: that id for each car cluster, in the order of tk_clusters
    int32_t* tk_prep;         // [N] per cluster region, parallel to tk_pairs: the id of the pair's label
    int8_t* cl_state;         // [N] per cluster root: Cluster::state (-1 untouched, 0 static, 1 dynamic)
    int32_t* tk_mbegin;       // [N] per car root: first slot of its members in tk_members (scan-local)
    int32_t* tk_cursor;       // [N] per car root: scatter cursor
    int32_t* tk_members;      // [N] per scan: apri indices of the car points, grouped by cluster
    int32_t* tk_hit;          // [N] per member slot: slot of the next table hit by the transformed point, or -1
    int32_t* tk_uniq;         // [N] per cluster region: sorted unique hit slots (sampleVec, ssc.cpp:1319-1321)
    int32_t* tk_nuniq;        // [N] per car root
    int2* tk_pairs;           // [N] per cluster region: (next label, unique voxels) = remap_name (ssc.cpp:1275,1304-1316)
    int32_t* tk_npairs;       // [N] per car root: remap_name.size()
    int32_t* tk_clusters;     // [N] per scan: roots of its car clusters, ascending
    int32_t* tk_scan;         // [B][4] per scan: car clusters, car points, dynamic clusters, dynamic points
    uint8_t* pt_dyn;          // [N] per apri point: SCVOD_DYN_*
    uint8_t* pt_mapcls;       // [N] per INPUT point, for the static map: kMap* bits
    // loader-side VoxelGrid
    int32_t* vg_par;          // [B][16] per scan: min_b[3], mul[3], overflow flag, kept points, distinct cells
    int32_t* vg_range;        // [1] largest cell index range of the batch
    int32_t* vg_outoff;       // [B+1] output offsets (uploaded by the host between the two phases)
    uint16_t* vb_lut;         // [B][kVgLutBins] monotone key-bin -> bucket table of the VoxelGrid run; nullptr in the hot path
    const int32_t* vb_lut_shift;  // device word: key >> *vb_lut_shift = bin (k_vg_lut derives it from the batch's index range)
    const uint32_t* vg_labels;    // VoxelGrid run only: per input point label (or nullptr) and the loader's intensity scale
    float vg_max_intensity;
};

struct TrackJob {          // scan-vs-next-scan probe
    const float4* pts;         // explicit cluster points, or nullptr when gathered from apri
    const int32_t* members;    // apri indices (batch mode) or nullptr
    const int32_t* pt_cluster_begin;  // [n_clusters+1] offsets into pts / members
    int32_t n_clusters;
    int32_t n_pts;
    // per cluster: which transform / which source scan / which next table
    const int32_t* cluster_pair;   // [n_clusters] pair index (0 for the single-pair API)
    const float* T;                // [n_pairs][12]
    const int32_t* pair_pt_begin;  // batch mode: [n_pairs+1] first point (offset into members) of every pair
    int32_t n_pairs, max_pair_pts;
    // next tables: explicit (single pair) or arena scans (batch)
    const int32_t* next_keys;      // explicit table or nullptr
    const int32_t* next_labels;    // explicit labels or nullptr (= all labelled)
    int32_t n_next_vox;
    // outputs
    int32_t* hit_slot;     // [n_pts]
    uint64_t* work;        // [n_pts] sort workspace
    int32_t* uniq_slots;   // [n_pts] per cluster region starts at pt_cluster_begin[c]
    int32_t* uniq_count;   // [n_clusters]
};

struct TrackBatch {            // scvod_batch_track: every scan of the batch against its successor
    const int32_t* next_scan;      // [B] successor of scan s: index in the batch, -1 = none, <= -2 = external table -2 - v
    const int4* const* ext_tables; // device array of external tables: record 0 = {n_voxels, 0, 0, 0}, then vox_track records
    int32_t n_ext;
    const float* T;                // [B][12] trans_next^-1 * trans_pre of (s, successor)
    float occupancy;               // ssc/occupancy_
};

// intensity merge of the clusters (SSC::refineClusterByIntensity, ssc.cpp:571-635; scvod_k_merge.inc).  Scratch of its own, allocated
// when a ctx turns the merge on: per-point arrays indexed base + i (names and voxel slots are scan-local and < n).
struct MergeJob {
    int32_t iterations, search_c;
    float diff, cov;             // ssc/intensity_diff_, ssc/intensity_cov_
    int32_t* vlab;               // [N] label (cluster name) of every voxel: that of its first point
    int32_t* key0;               // [N] per name: smallest voxel key of the cluster (sort1's key)
    int32_t* nxt;                // [N] per name: the cluster it was fused into (-1: never a member of a fusion)
    uint8_t* own;                // [N] per name: the cluster's own label is in its neighbour set S
    uint8_t* fz;                 // [N] per name: took part in a fusion as its target
    int32_t* qv;                 // [N] voxels with cov <= intensity_cov in key order ...
    int32_t* qk;                 // [N] ... and their keys
    uint32_t* box;               // [7 N] per fused name: box (order-preserving encoding) + member count
    uint64_t* pair;              // [kImPairsPerPt N + kImPairsPerScan B] (cluster << 32 | neighbour label) per scan
    uint64_t* cand;              // [N] clusters to visit: (~key << 32 | first pair)
    int32_t* pt_merged;          // [N] post-merge canonical name per apri point
    int32_t* stats;              // [8] clusters before, fusions, clusters after, scans with a fusion, scans whose pairs overflowed
};
constexpr int kImPairsPerPt = 4, kImPairsPerScan = 256;

// region growing of the large clusters (SSC::recognize / regionGrowing, ssc.cpp:797-860; scvod_k_rgrow.inc), opt-in.  One job per
// chunk of scans [s0, s0 + ns): chunk points are numbered g = scan_off[s] - off0 + i, stage positions p are the candidates' points
// in (scan, cluster, apri index) order.  Scratch (chunk capacity C points) and batch-wide outputs (indexed scan_off[s] + i).
struct RgJob {
    int32_t k, min_seg, max_seg;   // neighbours (<= 16), kept segment sizes
    float cos_t, curv_thr;         // cosf(smoothness), curvature threshold
    double frac;                   // building iff kept points >= n * frac
    int32_t s0, ns, from_apri;
    int64_t off0;                  // scan_off[s0]
    uint32_t* bmin;                // [3 C] per chunk point (as a cluster name): box minimum (order-preserving encoding)
    uint32_t* bmax;                // [3 C] ... maximum
    int32_t* bcnt;                 // [C] ... member count
    uint64_t* key_in;              // [C] (name << 32 | g) of the candidates' points, unused slots ~0
    uint64_t* key_out;             // [C] sorted
    int32_t* cnt;                  // [2] candidate points, candidate clusters of the chunk
    int2* cl;                      // [C] per cluster: first position, points
    int32_t* cl_name;              // [C] per cluster: its name (chunk point)
    float4* grid;                  // [2 C] per cluster: origin, cell size; cells per axis
    int32_t* cell;                 // [3 C] per cluster at 3 p0: CSR cell ends
    int32_t* pcell;                // [C] per position: its cell
    int32_t* cell_pts;             // [C] positions in cell order
    int32_t* pos_cl;               // [C] per position: cluster
    int2* pl;                      // [C] per position: scan, apri index
    float4* cxyz;                  // [C] per position: coordinates
    int32_t* nbr;                  // [k C] per position: the k_eff nearest positions of its cluster
    float4* nrm;                   // [C] per position: normal, curvature
    uint16_t* emask;               // [C] per position: valid edges to its neighbours
    uint64_t* lab;                 // [C] labels of the clusters on the HBM path
    int32_t* segc;                 // [C] per owner position: its segment's size
    int32_t* tail;                 // [C] per cluster: its tail points
    uint8_t* cls;                  // [N] per apri point: 0 erased, 1 tree, 2 car, 3 building
    float4* out_nc;                // [N] per apri point: normal, curvature (NaN for non-candidates)
    int32_t* out_seg;              // [N] per apri point: apri index of its segment's seed, -1 for non-candidates
    int32_t* stats;                // [8] see scvod_batch_region_growing_stats
};

// intensity calibration by incidence angle (SSC::intensityCalibrationByCurvature, ssc.cpp:98-153; scvod_k_calib.inc), opt-in.  One job
// per chunk of scans [s0, s0 + ns): chunk points are numbered g = scan_off[s] - off0 + i; a scan's non-ground cloud (n <= its points)
// occupies the first n slots of its range.  Scratch only (chunk capacity C points, at most kCalChunkScans scans): the stage's product is
// the patched Arena::apri_int; the per-point outputs exist for the scan a fetch asks for.
constexpr int kCalChunkScans = 65535;
struct CalJob {
    int32_t k;                     // neighbours (3..16)
    float max_int;                 // ssc/max_intensity_
    int32_t s0, ns;
    int64_t off0;                  // scan_off[s0]
    int32_t write_apri;            // 1: the calibrated value replaces apri_int of the points that passed the range/FOV test
    int32_t force_fallback;        // development (tools/intensity_calibration_cost.py): no tile staged, no LDS reserved, every query reads HBM
    float4* sxyz;                  // [C] per scan: {x, y, z, position} in cell order
    int32_t* pcell;                // [C] per position: its cell
    int32_t* cell;                 // [3 C + 4 kCalChunkScans] per scan at 3 g0 + 4 (s - s0): CSR cell ends
    int32_t* slot;                 // [C] per input point: its apri slot, -1 for the others
    float4* grid;                  // [2 kCalChunkScans] per scan: origin, cell edge; cells per axis, n
    float* out_int;                // [C] per position: calibrated intensity, or nullptr
    float4* out_nc;                // [C] per position: normal, curvature, or nullptr
    int32_t* stats;                // [8] see scvod_batch_intensity_calibration_stats, or nullptr (a fetch counts nothing)
    unsigned long long* cand;      // [1] candidates examined (with stats)
};

// export of a batch's result (scvod_batch_point_labels / scvod_batch_export_points; scvod_export.hip): one SCVOD_PT_* byte per INPUT
// point, and the kept points compacted in input order.  A scan is cut into tiles of kExpTile points (256 threads x 8 rounds, round u
// covers the points tile + u * 256 + thread); the tiles of scan s are tile_cnt[s * tiles_per_scan ..).  Scratch of its own (not the arena).
constexpr int kExpTile = 2048;
struct ExportJob {
    const uint8_t* labels;         // [total points] the label bytes the export reads (its own buffer, never the map's marks)
    uint32_t keep_mask;            // bit L set: points labelled L are kept
    const float* pose;             // [B][12] row-major 3x4 per scan, or nullptr: sensor frame
    const uint32_t* payload_in;    // [total points] or nullptr
    float4* out;                   // caller's buffers: nullptr = count only
    uint32_t* payload_out;         // or nullptr
    int32_t* src_out;              // or nullptr
    long long cap;                 // points the caller's buffers hold
    int32_t* out_off;              // [B + 1] caller's
    int32_t* tile_cnt;             // [B * tiles_per_scan] kept points per tile, then their exclusive prefix inside the scan
    int32_t* scan_cnt;             // [B] kept points per scan
    long long* stats;              // [4] points written, points kept, 1 = the output outgrew cap, 0
    int32_t tiles_per_scan;
};
void launch_point_labels(const Arena& A, uint8_t* labels, int use_dyn, hipStream_t st);
// the labels with the class of an apri point's cluster carried along (scvod_batch_point_classes): cls [N] per apri point, 3 = building
void launch_point_classes(const Arena& A, const uint8_t* cls, uint8_t* labels, int use_dyn, hipStream_t st);
void launch_export(const Arena& A, const ExportJob& J, hipStream_t st);

// scan stacking (scvod_batch_stack_scans; scvod_stack.hip): every (group, scan of its window) pair is a SEGMENT -- a contiguous run of
// input records that goes to a contiguous run of output records with one 3x4 matrix, or with none for the middle scan.  The host cuts
// the non-empty segments into tiles of kStackTile points (256 threads x 8 rounds, as the export's) and lists them: a workgroup owns one
// tile, so everything but the point itself is uniform over the workgroup.  Both tables live in scratch of their own (not the arena).
constexpr int kStackTile = 2048;
struct StackSeg {       // 64 bytes
    float T[12];        // row-major 3x4 (unused when copy != 0)
    int32_t in_base;    // first input record
    int32_t out_base;   // first output record
    int32_t n;          // records
    int32_t copy;       // 1: the middle scan, records handed on bit for bit
};
struct StackTile {
    int32_t seg;        // index into the segment table
    int32_t first;      // first record of the tile inside its segment (a multiple of kStackTile)
};
void launch_stack(const StackSeg* segs, const StackTile* tiles, int n_tiles, const float4* in, float4* out, const uint32_t* payload_in,
                  uint32_t* payload_out, int32_t* src_out, hipStream_t st);

// seen-through points (scvod_visibility_device / scvod_batch_visibility; scvod_visibility.hip): the host lists the kStackTile-point tiles
// of the non-empty scans, the scans and the (scan, viewer) pairs with their matrices; a workgroup owns one tile of ONE scan, so the
// image base and every matrix are uniform over it.  All tables live in scratch of their own (not the arena).
struct VisPair {        // 64 bytes
    float T[12];        // row-major 3x4: the query scan's frame -> the viewer's frame
    int32_t viewer;     // the viewer's scan (its image)
    int32_t pad[3];
};
struct VisScan {        // 16 bytes
    int32_t base;       // first record of the scan in the cloud
    int32_t n;          // records
    int32_t pair_begin; // first of its pairs in the pair table
    int32_t n_pairs;    // viewers
};
struct VisJob {
    BinParams bin;
    BinFast binfast;
    KeepFast keep;
    int32_t halo, min_through, vote_num, vote_den;
    float gap_abs, gap_rel;
    const float4* pts;
    const uint8_t* mask;               // per point, or nullptr: every point is a query
    const VisScan* scans;
    const VisPair* pairs;
    const StackTile* tiles;            // {scan, first record of the tile inside it}
    int32_t n_tiles;
    float* images;                     // [n_scans][azimuth_num * sector_num]
    uint32_t* votes;                   // per point or nullptr
    uint8_t* verdict;                  // per point or nullptr
    unsigned long long* scan_counts;   // [n_scans][6] or nullptr
    unsigned long long* counters;      // [8]: the six sums
};
void launch_vis_image(const VisJob& J, hipStream_t st);
void launch_vis_vote(const VisJob& J, hipStream_t st);
// mask[scan_off[s] + nonground_idx[..]] = 1 for the non-ground list of every scan of the batch (the mask is cleared before)
void launch_vis_mask(const Arena& A, uint8_t* mask, hipStream_t st);
// host only: the stage's parameter check and the viewer lists (begin [n_scans + 1], viewers); SCVOD_OK or SCVOD_ERR_INVALID
int vis_check_params(const scvod_visibility_params* p);
int vis_viewers(const int32_t* h_next_scan, int n_scans, int before, int after, std::vector<int32_t>& begin, std::vector<int32_t>& viewers);

// a world-frame cloud against the range images of every scan (scvod_cloud_visibility_device; scvod_cloudvis.hip): the points are keyed by
// a coarse world tile and sorted, a workgroup owns one chunk of kCvisChunk consecutive sorted points and walks all scans, skipping those
// whose image no point of the chunk can lie in.  Scratch of its own (not the arena, not the scan stage's).
constexpr int kCvisThreads = 64;                // one wave per chunk: its bound is as tight as 512 neighbouring points allow
constexpr int kCvisChunk = 8 * kCvisThreads;    // 8 records per thread stay in registers, as in the scan stage's tile
struct CvisJob {
    VisJob V;                          // grid, window, gaps and vote rule as vis_pair reads them (the scan stage's pointers stay 0)
    float max_range;                   // 0: the grid's max_dis alone
    float reach;                       // min(max_dis, max_range): a pair with dis' beyond it is OUTSIDE
    const float4* pts;                 // [n] world frame
    long long n;
    const uint32_t* order;             // [n] the sorted index list, or nullptr: the input order
    const float* T;                    // [n_scans][12] world -> viewer
    const float* images;               // [n_scans][azimuth_num * sector_num]
    int32_t n_scans;
    uint16_t* votes;                   // [n][4] or nullptr
    uint8_t* verdict;                  // [n] or nullptr
    unsigned long long* counters;      // [10] scvod_cloud_visibility_stats
};
size_t cvis_sort_bytes(long long n);   // rocprim's temporary storage for n (key, index) pairs
void launch_cvis_key(const float4* pts, long long n, uint32_t* key, uint32_t* idx, hipStream_t st);
hipError_t launch_cvis_sort(void* tmp, size_t tmp_bytes, const uint32_t* key_in, uint32_t* key_out, const uint32_t* idx_in, uint32_t* idx_out,
                            long long n, hipStream_t st);
void launch_cvis_vote(const CvisJob& J, hipStream_t st);
int cvis_check_params(const scvod_cloud_visibility_params* p);  // host only: SCVOD_OK or SCVOD_ERR_INVALID

// the clusters of a batch as an object table (scvod_batch_objects; scvod_objects.hip).  Tiles as in the export, over the APRI points of a
// scan; per tile two words {objects, member points}, the first turned into its exclusive prefix inside the scan.  Scratch of its own (not
// the arena): per point of the ctx's capacity unless stated.
struct ObjectJob {
    int32_t use_track;             // 0: SCVOD_OBJ_NO_TRACK (state -1, dynamic 0 everywhere)
    const uint8_t* cls;            // [N] per apri point: 1 tree / other, 2 car, 3 building (the region growing's bytes when it ran, else pt_type)
    scvod_object* out;             // caller's buffers: nullptr = no records
    long long cap_obj;
    int32_t* obj_off;              // [B + 1] caller's
    int32_t* member_src;           // or nullptr
    long long cap_mem;
    int32_t* point_object;         // [total points] or nullptr; cleared to -1 by the caller of launch_objects
    int32_t* tile_cnt;             // [2 B tiles_per_scan]
    int32_t* scan_cnt;             // [2 B] objects, member points per scan
    long long* stats;              // [4] objects written, objects found, member slots needed, 1 = a buffer was outgrown
    uint64_t* key_in;              // [N] (object << 32 | apri position) per slot, upper word ~0 for a point of no object; nullptr: count only
    uint64_t* key_out;             // [N] sorted on the object bits: [0, members) is the member list
    int32_t* root_obj;             // [N] per object root (scan_off[s] + name): its index in the table
    int32_t* begin;                // [N + 1] per object: first slot of its run in key_out; [objects] = members
    int32_t* nvox;                 // [N] per object: occupy_voxels.size()
    int32_t tiles_per_scan;
};
int obj_sort_bits(long long total_pts);
size_t obj_sort_bytes(long long cap_pts);  // temporary storage of the radix sort of a batch's keys
hipError_t launch_objects(const Arena& A, const ObjectJob& J, void* sort_tmp, size_t sort_bytes, hipStream_t st);  // (the sort's status)
// eigenvalue descriptor of the table's objects (scvod_batch_object_shapes): reads key_out, begin and stats[1] of the ObjectJob that
// built the table -- the ctx's scratch; none of the table call's caller buffers
struct ShapeJob {
    const uint64_t* key_out;     // the table's sorted member list
    const int32_t* begin;        // the table's run starts
    const long long* tab_stats;  // the table's stats ([1]: its objects)
    ObjShape* out;     // [cap] caller's
    long long cap;
    long long* stats;  // [4] records written, objects of the table, written records with flags bit 0, 1 = the table outgrew cap
    FeatureParams K;
};
void launch_object_shapes(const Arena& A, const ShapeJob& J, hipStream_t st);
// ESF descriptor of grouped points (scvod_esf_device / scvod_batch_object_esf; scvod_objesf.hip).  The batch form first gathers the
// table's members and the objects' classes into the stage's scratch (launch_esf_gather), so the kernel reads one layout.
constexpr int kEsfCachePts = 3584;      // points of an object kept in LDS (SCVOD_ESF_CACHE_POINTS): two workgroups fit a CU
struct EsfJob {
    const float4* pts;                  // xyzi records
    const int32_t* begin;               // [objects + 1]
    long long n_host;                   // objects, when n_dev is nullptr
    const long long* n_dev;             // the table's stats ([1]: its objects) or nullptr
    const uint8_t* obj_cls;             // [objects] or nullptr: no mask
    uint32_t cls_mask;
    int32_t samples, min_points;
    uint32_t seed;
    ObjEsf* out;                        // [cap] caller's
    float* sig;                         // [cap][640] caller's, or nullptr
    long long cap;
    uint8_t* sample_bytes;              // [blocks][samples] per workgroup: what sweep 1 leaves for sweep 2
    unsigned long long* counters;       // [8] scvod_esf_stats; [8] the next object to take
    int32_t blocks;
};
size_t esf_work_bytes(int blocks, int samples);
void launch_esf(const EsfJob& J, hipStream_t st);
// the batch form's gather: member slot p of the table -> pts_out[p] (the point obj_load reads), object o -> cls_out[o]
void launch_esf_gather(const Arena& A, const uint64_t* key_out, const int32_t* begin, const long long* tab_stats, const uint8_t* cls,
                       float4* pts_out, uint8_t* cls_out, hipStream_t st);

typedef void (*TimerHook)(void* user, const char* name, int begin);

// Launches.  `th`/`tu` optional per-kernel timing hook (called before and after each launch).
// do_patchwork: 1 = Patchwork + fused binning, 0 = binning of the input cloud in input order,
// 2 = neither (apri / counts already in the arena: voxel stage only), 4 = the voxel stage alone on the compact arrays a
// do_patchwork = 1 call without voxels left (the intensity calibration runs between the two).
void launch_process(const DevParams& P, const Arena& A, hipStream_t st, int do_patchwork, int apply_filter,
                    int do_voxels, TimerHook th, void* tu, int lean_voxels = 0, int lean_emit = 0);
// lean_voxels = 1: the voxel stage leaves vox_av / vox_cov unwritten; launch_vox_descriptors fills them for scans [s0, s0 + n_scans)
// from vox_pt_begin / vox_pts / apri_int when somebody asks
void launch_vox_descriptors(const Arena& A, int s0, int n_scans, hipStream_t st, TimerHook th, void* tu);
// lean_emit = 1 (do_patchwork = 1 only; the caller checked idx3_roundtrip_ok): the arrange pass stages the kept points' index triples
// in zkey, k_emit compacts them without fetching a point and leaves apri_int unwritten; launch_apri_intensity fills it for the batch
void launch_apri_intensity(const Arena& A, hipStream_t st, TimerHook th, void* tu);
// ... and writes none of ground_idx / nonground_idx / rejected_src; launch_emit_lists fills the three for the batch from order,
// order_off, patch_rec, emit_off and seg
void launch_emit_lists(const Arena& A, hipStream_t st, TimerHook th, void* tu);
void launch_apri_expand(const DevParams& P, const Arena& A, int s0, int n_scans, int max_pts, hipStream_t st);
struct VgJob {                // SSC::getCloud label filter + pcl::VoxelGrid (ssc.cpp:1063-1076, 1103-1106)
    const uint32_t* labels;   // per input point, or nullptr (no filter, no intensity scaling)
    float max_intensity;
    float inv_leaf[3];        // 1.f / leaf, fp32 like Eigen::Array4f::Ones() / leaf_size_
    float4* out;              // caller's output buffer
};
void launch_voxelgrid_keys(const Arena& A, const VgJob& J, hipStream_t st);
void launch_voxelgrid_lut(const Arena& A, hipStream_t st);
void launch_voxelgrid_gather(const DevParams& P, const Arena& A, const VgJob& J, long long out_capacity, hipStream_t st);
void launch_cls(const Arena& A, int s, size_t scan_base, int n_points, hipStream_t st);
void launch_cluster(const DevParams& P, const Arena& A, int from_apri, hipStream_t st, TimerHook th, void* tu);
size_t merge_lds_bytes(const DevParams& P, int max_scan_pts);  // dynamic LDS of k_im_merge: row starts + invalid bitmap
void launch_merge(const DevParams& P, const Arena& A, const MergeJob& M, int from_apri, hipStream_t st, TimerHook th, void* tu);
size_t rg_sort_bytes(int chunk_pts);  // temporary storage of the radix sort of a chunk's keys
void launch_rgrow(const DevParams& P, const Arena& A, const RgJob& J, int chunk_pts, void* sort_tmp, size_t sort_bytes, hipStream_t st,
                  TimerHook th, void* tu);
void launch_calib(const Arena& A, const CalJob& J, int chunk_pts, hipStream_t st, TimerHook th, void* tu);
void launch_calib_apri(const Arena& A, int s, int n_apri, hipStream_t st);  // the calibrated intensity into scan s's PointAPRI records
void launch_merge_lastname(const Arena& A, const MergeJob& M, hipStream_t st, TimerHook th, void* tu);  // carrier of max_name -> its fusion
void launch_lastname(const DevParams& P, const Arena& A, hipStream_t st, hipStream_t st2, hipStream_t st3, hipEvent_t ev_fork, hipEvent_t ev_join2,
                     hipEvent_t ev_join3, TimerHook th, void* tu);
void launch_track(const DevParams& P, const Arena& A, const TrackJob& J, int batch_mode, hipStream_t st,
                  TimerHook th, void* tu);
struct ChainJob;
void launch_track_batch(const DevParams& P, const Arena& A, const TrackBatch& J, int from_apri, int phases, hipStream_t st,
                        TimerHook th, void* tu, const ChainJob* chain = nullptr, hipEvent_t before_chain = nullptr);
void launch_track_dyn(const Arena& A, int from_apri, hipStream_t st);  // per-point bytes from the cluster states (again, after a resume)
void launch_export_table(const Arena& A, int s, int4* out, long long cap_records, hipStream_t st);
void launch_nn(const float* map_xyz, int32_t n_map, const float* q_xyz, int32_t n_q, float radius, int32_t* nn_idx,
               float* nn_sq, uint8_t* within, const float origin[3], float cell, int32_t buckets, int* work, int bounded,
               hipStream_t st);
// exclusive scan of `n` ints on `st` (three k_scan_* launches): out[i] = in[0] + .. + in[i - 1], *grand_total = the sum;
// block_tot: (n + 1023) / 1024 ints of scratch
void launch_scan_ints(const int* in, int* out, int* block_tot, int* grand_total, int n, hipStream_t st);

// the CSR hash grid that the nearest-neighbour stages share (scvod_grid.h).  grid_buckets: the power of two for a cloud of n points;
// grid_work_ints: the ints of `work` behind a grid.  grid_build enters the points xyz[stride * i] (keep: nullptr, or a point whose byte
// is 0 is not entered) on `st` -- two memsets, k_grid_count, launch_scan_ints, k_grid_fill -- and returns what a query kernel reads;
// n <= 0: the view alone, nothing is launched and no query may read it
struct PointGrid;
int32_t grid_buckets(int32_t n);
size_t grid_work_ints(int32_t buckets, int32_t n);
PointGrid grid_build(const float* xyz, int stride, const uint8_t* keep, int32_t n, const float origin[3], float cell, int32_t buckets, int* work,
                     hipStream_t st);

// evaluation against labelled truth (scvod_evaluate_device / scvod_batch_evaluate / scvod_classify_map_device; scvod_eval.hip).  A grid is
// the shared one over the estimate cloud, in `work` (grid_work_ints ints); counters: 8 words, cleared by every launch
struct EvClasses {  // the semantic classes (label & 0xFFFF) that count as dynamic
    int32_t n;
    uint16_t c[16];
};
// counters: gt static, gt dynamic, est static, est dynamic, preserved, static preserved, dynamic preserved, 0.  est_keep: nullptr or one
// byte per estimate point (0: not part of the estimate).  point_result: nullptr or one byte per gt point
void launch_eval(const float* gt_xyz, const uint32_t* gt_label, int32_t n_gt, const float* est_xyz, const uint32_t* est_label,
                 const uint8_t* est_keep, int32_t n_est, double limit, const EvClasses& K, float cell, int32_t buckets, int* work,
                 unsigned long long* counters, uint8_t* point_result, hipStream_t st);
// per input point of the arena's batch: packed world xyz (pose: [B][12] device) and keep = bit labels[p] of keep_mask
void launch_eval_world(const Arena& A, const uint8_t* labels, uint32_t keep_mask, const float* pose, float* world_xyz, uint8_t* keep,
                       hipStream_t st);
// counters: points of class 0 (unmatched), 1 .. 4 (metric.py's TP_STATIC .. FN_DYNAMIC), 0, 0, 0.  cls: nullptr or one byte per point
void launch_classify(const float* orig_xyz, const uint8_t* pred_static, int32_t n, const float* static_xyz, int32_t n_static,
                     const float* dynamic_xyz, int32_t n_dynamic, float r15, float r10, float cell, int32_t buckets_s, int* work_s,
                     int32_t buckets_d, int* work_d, unsigned long long* counters, uint8_t* cls, hipStream_t st);

// class scores against labelled truth (scvod_score_classes_device / scvod_batch_score_classes; scvod_classes.hip).  The grid is the
// shared one (grid_buckets, grid_work_ints) with the caller's cell edge; work: cs_work_bytes bytes; counters: 24 words, cleared by every
// launch: conf[4][5] row-major, pd_far, the pass-2 list's length, 0, 0.  est_class: one SCVOD_PT_* byte per estimate point
struct CsLists {  // the semantic classes (label & 0xFFFF) of ground / building / tree truth points
    int32_t n_ground, n_building, n_tree;
    uint16_t ground[8], building[8], tree[8];
};
size_t cs_work_bytes(int32_t buckets, int32_t n_est, int32_t n_gt);
void launch_class_score(const float* gt_xyz, const uint32_t* gt_label, int32_t n_gt, const float* est_xyz, const uint8_t* est_class,
                        const uint8_t* est_keep, int32_t n_est, const CsLists& L, float cell, float max_dist, int32_t rings, int32_t buckets,
                        int* work, unsigned long long* counters, uint8_t* point_result, hipStream_t st);

// the points of a labelled cloud grouped by their 32-bit key (scvod_score_instances_device; scvod_instances.hip).  work: in_work_bytes(cap)
// bytes (the global table of in_table_slots(cap) slots, the sort's buffers); counters: 8 words, cleared by every launch: records written,
// distinct keys found, overflow, spilled tiles, then the kernels' own.  out: nullptr counts only.  variant 0: equal keys of a wave are
// combined before the LDS table (the shipped path); 1: every point adds into the LDS table on its own (tools/instance_score_cost.py's
// comparison).  Returns 0 or the hipError_t of the sort
uint32_t in_table_slots(int32_t cap);
size_t in_work_bytes(int32_t cap);
int launch_instance_score(const uint32_t* key, const uint8_t* point_result, int32_t n, scvod_instance* out, int32_t cap, int64_t* d_n, void* work,
                          unsigned long long* counters, int variant, hipStream_t st);

// the truth label every object of the table covers (scvod_batch_object_truth; scvod_objtruth.hip): reads key_out, begin and stats[1] of
// the ObjectJob that built the table, as ShapeJob does.  work: truth_work_bytes bytes (the spill list, then kOtGroups regions of
// 2 * max_scan_pts slots); counters: the 8 words of scvod_batch_object_truth_stats, cleared by every launch
constexpr int kOtGroups = 32;  // workgroups of the fallback launch, each with a region of its own
enum { kOtWritten = 0, kOtObjects, kOtOverflow, kOtFallback, kOtMovingPoints, kOtMovingMembers };
struct TruthJob {
    const uint64_t* key_out;     // the table's sorted member list
    const int32_t* begin;        // the table's run starts
    const long long* tab_stats;  // the table's stats ([1]: its objects)
    const uint32_t* gt;          // [total points] caller's labels, one per input point
    EvClasses K;                 // the moving classes
    scvod_object_truth* out;     // [cap] caller's
    long long cap;
    unsigned long long* counters;
    // filled by launch_object_truth
    int32_t* list;               // objects for the fallback, in arbitrary order
    long long list_cap;
    unsigned long long* regions;
    long long region_slots;
};
size_t truth_work_bytes(long long total_pts, int max_scan_pts);
void launch_object_truth(const Arena& A, TruthJob J, void* work, hipStream_t st);

// the objects of the table vote on the seen-through verdict (scvod_batch_object_visibility; scvod_objvis.hip): reads key_out, begin and
// stats[1] (objects) / stats[2] (members) of the ObjectJob that built the table.  work: objvis_work_bytes bytes (8 words per tile of
// SCVOD_OBJVIS_TILE list positions, cleared by every launch); counters: the 8 words of scvod_batch_object_visibility_stats, cleared by
// every launch
enum { kOvStObjects = 0, kOvStVoted, kOvStForced, kOvStSeen, kOvStMovedSeen, kOvStMovedKeep, kOvStWritten, kOvStOverflow };
struct ObjVisJob {
    const uint64_t* key_out;       // the table's sorted member list: object << 32 | batch slot
    const int32_t* begin;          // the table's run starts
    const long long* tab_stats;    // the table's stats
    const uint8_t* verdict;        // [total points] caller's verdict bytes
    const uint32_t* votes;         // [total points] caller's pair counters, or nullptr
    const unsigned char* obj_bytes;  // the caller's scvod_object records (SCVOD_OBJVIS_WITH_TRACK), or nullptr
    uint8_t* out;                  // [total points] caller's, may be `verdict`, or nullptr
    scvod_object_visibility* rec;  // [cap] caller's, or nullptr
    long long cap;
    int32_t pool, min_points, min_tested, min_through, vote_num, vote_den;
    unsigned long long* counters;
    unsigned* acc;                 // filled by launch_object_visibility
};
size_t objvis_work_bytes(long long total_pts);
void launch_object_visibility(const Arena& A, ObjVisJob J, void* work, hipStream_t st);

// the objects of a table linked into tracks (scvod_object_tracks_device / scvod_batch_object_tracks; scvod_tracks.hip).  work:
// trk_work_bytes bytes; its first trk_tables_bytes hold the pose matrices [n_scans][12] and the successor table [n_scans], each rounded
// up to 256 bytes, staged by the caller.  counters: the 8 words of scvod_object_tracks_stats, cleared by the caller on the stream
enum { kTrkStObjects = 0, kTrkStFound, kTrkStWritten, kTrkStKind1, kTrkStKind2, kTrkStRefused, kTrkStLongest, kTrkStOverflow };
struct TrkJob {
    const scvod_object* objects;   // caller's records
    const int32_t* obj_off;        // [n_scans + 1] caller's offsets (device); the batch form: made from the table's scan counts
    int32_t n_scans;
    long long cap;                 // records the caller vouches for (cap_links)
    const int32_t* cand_begin;     // [objects + 1] and
    const int2* cand;              //   (successor object, count): the caller's overlap candidates, or nullptr
    const int32_t* root_obj;       // batch form: the table's root_obj; the candidates are the arena's remap_name pairs then
    int32_t flags, min_points, min_length;
    float occupancy, gate2, size_ratio;  // gate2 = gate * gate in fp32
    scvod_object_link* out_links;  // caller's outputs, each may be nullptr
    scvod_track* out_tracks;
    long long cap_tracks;
    int32_t* out_tobj;
    int32_t* n_tracks;
    unsigned long long* counters;
    // filled by launch_object_tracks: slices of `work`
    const float* T;
    const int32_t* next;
    float4* cw;                    // world centre, box diagonal
    unsigned long long *slot, *prop_key, *chain, *val, *pre;
    scvod_object_link* links;
    int32_t *prop_b, *rank[2], *jump[2], *tobj, *heads;
};
int trk_rounds(int n_scans);  // pointer-jumping rounds: ceil(log2(max(n_scans, 2)))
size_t trk_tables_bytes(int n_scans);
size_t trk_work_bytes(long long cap, int n_scans);
hipError_t launch_object_tracks(const Arena& A, TrkJob J, const int32_t* scan_cnt, void* work, hipStream_t st);

// the tracks of a table vote on the seen-through verdict (scvod_track_visibility_device; scvod_trackvis.hip).  work: tv_work_bytes
// bytes; its first tv_tables_bytes hold the pose matrices [n_scans][12], staged by the caller.  counters: the 8 words of
// scvod_track_visibility_stats, cleared by the caller on the stream
enum { kTvStObjects = 0, kTvStTracks, kTvStVoted, kTvStMotion, kTvStCleared, kTvStToSeen, kTvStToKeep, kTvStLatch };
struct TvJob {
    const scvod_object* objects;          // caller's tables, read only
    const int32_t* obj_off;               // [n_scans + 1]
    int32_t n_scans;
    long long cap;                        // records of objects / links / tobj the caller vouches for
    const scvod_object_link* links;
    const scvod_track* tracks;
    long long cap_tracks;
    const int32_t* tobj;
    const int32_t* n_tracks;
    const scvod_object_visibility* ovis;  // or nullptr
    const int32_t* point_object;          // or nullptr (then out is nullptr too)
    const uint8_t* verdict;               // or nullptr: every byte SCVOD_VIS_UNTESTED
    uint8_t* out;                         // or nullptr: records only
    long long n_points;
    int32_t flags, window, min_length, min_moved, min_flagged, vote_num, vote_den;
    float travel2_min;                    // min_travel * min_travel in fp32
    scvod_track_vote* out_tracks;         // caller's records, each may be nullptr
    long long cap_tvotes;
    scvod_object_track_vote* out_objs;
    long long cap_ovotes;
    unsigned long long* counters;
    // filled by launch_track_visibility: slices of `work`
    const float* T;
    float4* cw;                           // world centre
    float* trav;                          // travel2
    unsigned char *mf, *vb;               // bit 0 flagged, bit 1 moved; the verdict byte (0xFF none), slot `cap`: always none
    int4* tdec;                           // per listed track: state, how, n_moved
};
size_t tv_tables_bytes(int n_scans);
size_t tv_work_bytes(long long cap, long long cap_tracks, int n_scans);
hipError_t launch_track_visibility(TvJob J, void* work, hipStream_t st);

// a map split by nearest-neighbour hits (scvod_map_split_device; scvod_split.hip).  The grid is the shared one (grid_buckets, grid_work_ints)
// over the base cloud with the caller's cell edge; work: sp_work_bytes bytes; stats: the 8 words of scvod_map_split_stats, written by
// every launch.  The optional outputs of SpJob are nullptr when not asked for; mark == nullptr: a byte array inside `work`
constexpr int kSpTile = 2048;  // base points per tile of the partition (k_exp_count's)
struct SpJob {
    const float* base;
    const uint32_t* base_label;
    const float* query;
    int32_t n_base, n_query, base_stride, query_stride, max_rings, n_reject;
    uint16_t reject[16];
    uint8_t* mark;
    int32_t* order;
    int64_t* seg4;
    float* base_out;
    const uint32_t* payload_in;
    uint32_t* payload_out;
    int32_t* nn_idx;
    float* nn_sq;
    // filled by launch_map_split: the lists of the second and the third pass
    int *n_list1, *list1_q, *list1_bi;
    float* list1_best;
    int *n_list2, *list2_q;
};
size_t sp_work_bytes(int32_t buckets, int32_t n_base, int32_t n_query);
void launch_map_split(SpJob J, float cell, int32_t buckets, void* work, unsigned long long* stats, hipStream_t st);

}  // namespace scvod
#endif
