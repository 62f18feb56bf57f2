// scvod_capi.hip -- the extern "C" boundary of libscvod.so (declared in include/scvod.h).
// Owns the device arena, host staging and the HIP stream; no torch types, no exceptions
// across the boundary.  GPU-only: every entry point fails loudly without a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../../include/scvod.h"
#include <algorithm>
#include "scvod_kernels.h"
#include "scvod_chain.h"
extern "C" void scvod__register_free(void* state);  // scvod_register.hip
extern "C" void scvod__normals_free(void* state);   // scvod_normals.hip

using namespace scvod;

namespace {

struct TimingEntry {
    const char* name;
    hipEvent_t e0, e1;
};

}  // namespace

struct UploadSlot {
    void* pinned = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
};

// a grow-only device block and the stream of the last call that used it (scratch_reserve waits for it before the block moves)
struct Scratch {
    void* buf = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    bool ran = false;
};

struct scvod_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    scvod_params params;
    scvod_pw_params pw;
    DevParams dev;
    int64_t cap_pts = 0;
    int32_t cap_scans = 0;
    void* arena_base = nullptr;
    size_t arena_bytes = 0;
    Arena A;             // carved pointers (pts / scan_off filled per call)
    float4* d_in = nullptr;        // ctx-owned input buffer for the per-scan host API
    int32_t* d_scan_off = nullptr; // [cap_scans+1]
    // tracking buffers
    float4* t_pts = nullptr;
    int32_t* t_hit = nullptr;
    uint64_t* t_work = nullptr;
    int32_t* t_uniq = nullptr;
    int32_t* t_begin = nullptr;
    int32_t* t_pair = nullptr;
    int32_t* t_pairpt = nullptr;
    uint16_t* d_vb_lut = nullptr;   // A.vb_lut is set only for the duration of a VoxelGrid run
    uint32_t* d_labels = nullptr;   // staging of the host API's label array (scvod_voxelgrid): side buffer
    scvod_apri* d_apri = nullptr;   // PointAPRI records: side buffer (Arena::apri)
    size_t side_bytes = 0;          // what ensure_side allocated so far (counted in scvod_arena_bytes)
    int32_t* t_count = nullptr;
    float* t_T = nullptr;
    int32_t* d_next_scan = nullptr;   // [cap_scans] successor table of scvod_batch_track
    const int4** d_ext = nullptr;     // [cap_scans] external (boundary) tables
    std::vector<float> up_T;          // what the device copies of T / next_scan / ext currently hold (re-uploaded on change only)
    std::vector<int32_t> up_next;
    std::vector<const void*> up_ext;
    UploadSlot up_ring[8];                   // (a chain-mode scvod_batch_track can upload six changed tables in one call: ADVICE r3)
    int n_cu = 256;                          // compute units of the device (hipDeviceProp: the chain plans one segment per CU)
    int up_next_slot = 0;
    bool track_valid = false;
    // sequential tracking chain (scvod_chain.hip)
    int track_mode = SCVOD_TRACK_CHAIN;
    int chain_seg = 0, chain_warm = -1;      // steps per segment (0: from the job, ~250 segments), warm-up steps in front of it (-1: chosen per stream, below)
    // warm-up chosen per job: 10 steps to begin with; when a batch walked more than a few segments again (its warm-up did not
    // reproduce their start states) the next batch of the stream warms up 2 steps longer, up to 16.  The counters come back through
    // a pinned word and an event: never a stream drain.
    int chain_warm_auto = 10, chain_warm_used = 10;
    int32_t* h_chain_fb = nullptr;           // pinned [8]
    hipEvent_t chain_fb_ev = nullptr;
    bool chain_fb_pending = false;
    int chain_fb_segments = 0;
    int chain_seg_used = 0;
    bool chain_generic = false;              // testing: every step through the generic (HBM-resident) step function
    bool max_name_literal = true;            // ssc.cpp:354: a frame's first new cluster re-uses the last running number (scvod_lastname.hip)
    bool last_name_valid = false;
    int32_t* d_chain_scans = nullptr;        // [cap_scans]
    ChainWalker* d_chain_walkers = nullptr;  // [cap_scans]
    int32_t* d_chain_fw = nullptr;           // [cap_scans + 1]
    int32_t* d_chain_stats = nullptr;        // [8]
    int32_t* d_step_ticks = nullptr;         // [cap_scans] per frame of the chain plan: what k_tk_chain spent in the step that starts there (ChainJob::step_ticks)
    int32_t* h_step_ticks = nullptr;         // pinned copy of the last batch's, behind step_fb_ev
    hipEvent_t step_fb_ev = nullptr;
    bool step_fb_pending = false;
    std::vector<int32_t> step_fb_scans;      // the plan (frames of every chain) the ticks in flight belong to
    std::vector<int32_t> step_ticks, step_ticks_scans;  // the last ticks that arrived and their plan
    std::vector<int32_t> plan_scans_tmp;
    std::vector<std::vector<int>> cuts_cache;  // the time-balanced segment starts of the plan below
    std::vector<int32_t> cuts_scans;
    std::vector<int> cuts_chain_first, cuts_chain_len;  // (two successor tables can flatten to the same frames and still split them differently)
    std::vector<uint8_t> cuts_halo;
    int cuts_warm = -1;
    int chain_balance = 1;                   // 1: cut the segments of a stream's next batch by these times (scvod_set_track_mode: segment_steps 0)
    int32_t* d_chain_cmp = nullptr;          // [1] scvod_batch_track_compare
    std::vector<uint8_t> halo;               // per scan of a batch: 1 = halo (warmed up over, never decided): scvod_set_track_owned / _halo
    ChainJob last_cj;                        // the chain job of the last scvod_batch_track (export / resume)
    TrackBatch last_tb;
    const unsigned char** d_ext_state = nullptr;  // [cap_scans] device array of the states a resume compares with
    void** h_ext_state_pin = nullptr;        // pinned staging of that table (scvod_batch_track_compare_device)
    bool ext_state_pin_valid = false;
    int ext_state_pin_n = 0;
    std::vector<int32_t> up_chain_scans, up_chain_fw, up_chain_walkers;
    void* chain_ws = nullptr;                // walkers' workspace (own allocation, grows on demand)
    size_t chain_ws_bytes = 0;
    ChainWs chain_geom;
    int chain_geom_pts = -1;                 // max_scan_pts the geometry was laid out for
    int64_t chain_pool_points = 0, chain_geom_pool = -1;  // appended-cloud capacity of a walker (0: 8 x the largest scan)
    bool chain_ran = false;                  // the last scvod_batch_track ran the chain (stats are meaningful)
    bool chain_ws_clean = false;
    int chain_ws_layout_pts = -1;
    bool tables_valid = false;   // successor tables (vox_track) built for the current clustering
    // intensity merge (scvod_set_intensity_merge, scvod_k_merge.inc): setting, scratch (own allocation, first merged clustering)
    int32_t im_iterations = 0, im_search_c = 2;
    float im_diff = 50.f, im_cov = 20.f;
    void* im_buf = nullptr;
    size_t im_bytes = 0;
    MergeJob im{};
    bool merged = false;         // the last clustering applied the merge: A.pt_cluster points at the fused partition (im.pt_merged)
    int32_t* pt_cluster_own = nullptr;  // the arena's own pt_cluster (the clustering's output and scratch, the max_name pass's input)
    int im_overflow = -1;        // scans of the last merged clustering whose neighbour pairs outgrew their scratch (-1: not read yet)
    // region growing of the large clusters (scvod_set_region_growing, scvod_k_rgrow.inc): setting, chunk scratch, batch-wide outputs
    bool rg_on = false;
    int32_t rg_k = 10, rg_min_seg = 20;
    float rg_cos = 0.f, rg_curv = 1.2f;
    double rg_frac = 0.2;
    void* rg_buf = nullptr;      // chunk scratch (capacity rg_cap points), grown when a chunk needs more
    size_t rg_buf_bytes = 0;
    int64_t rg_cap = 0;
    void* rg_out = nullptr;      // per apri point: class byte, normal + curvature, segment (the ctx's capacity)
    size_t rg_out_bytes = 0;
    RgJob rg{};
    void* rg_sort_tmp = nullptr;
    size_t rg_sort_bytes = 0;
    hipEvent_t rg_ev = nullptr;
    bool rg_done = false;        // the region growing ran on the current clustering (scvod_batch_cluster_types)
    // intensity calibration by incidence angle (scvod_set_intensity_calibration, scvod_k_calib.inc): setting, chunk scratch, the
    // buffers of a fetch (one scan)
    bool cal_on = false;
    int32_t cal_k = 10;
    float cal_max = 200.f;
    void* cal_buf = nullptr;     // chunk scratch (capacity cal_cap points) + counters, grown when a chunk needs more
    size_t cal_buf_bytes = 0;
    int64_t cal_cap = 0;
    void* cal_fetch = nullptr;   // normal + curvature and calibrated intensity of the scan a fetch asked for (cal_fetch_cap points)
    size_t cal_fetch_bytes = 0;
    int64_t cal_fetch_cap = 0;
    CalJob cal{};
    bool cal_done = false;       // the stage ran on the current batch
    // export of the result (scvod_batch_point_labels / scvod_batch_export_points, scvod_export.hip): scratch of its own, allocated by
    // the first export and NOT counted by scvod_arena_bytes
    uint8_t* exp_labels = nullptr;   // [cap_pts] the label bytes the compaction reads
    int32_t* exp_scan_cnt = nullptr; // [cap_scans]
    float* exp_pose = nullptr;       // [cap_scans][12]
    long long* exp_stats = nullptr;  // [4]
    int32_t* exp_tiles = nullptr;    // [exp_tiles_cap] tile counts / prefixes, grown when a batch needs more
    size_t exp_tiles_cap = 0;
    std::vector<float> exp_up_pose;  // what exp_pose holds
    hipStream_t exp_stream = nullptr;  // stream of the last export (scvod_batch_export_stats waits for it)
    bool exp_ran = false;
    // object table (scvod_batch_objects, scvod_objects.hip): scratch of its own, the small part allocated by the first call, the per-point
    // part by the first call that asks for more than the counts; not part of the arena
    int32_t* obj_scan_cnt = nullptr;  // [cap_scans][2]
    long long* obj_stats = nullptr;   // [4]
    int32_t* obj_tiles = nullptr;     // [obj_tiles_cap][2], grown when a batch needs more
    size_t obj_tiles_cap = 0;
    uint64_t* obj_keys = nullptr;     // [2 cap_pts] keys in, keys out
    int32_t* obj_words = nullptr;     // [3 cap_pts + 1] root_obj, nvox, begin
    void* obj_sort_tmp = nullptr;
    size_t obj_sort_bytes = 0;
    int64_t obj_bytes = 0;
    hipStream_t obj_stream = nullptr;  // stream of the last call (scvod_batch_objects_stats waits for it)
    bool obj_ran = false;
    // eigenvalue descriptor of the table's objects (scvod_batch_object_shapes): it reads the sorted member keys and the run starts the
    // last table call with lists left in obj_keys / obj_words, so it has to know which clustering they belong to
    uint64_t cluster_serial = 0;      // counts the clusterings this ctx published
    uint64_t obj_lists_serial = 0;    // the clustering whose lists the scratch holds; 0: none
    int obj_lists_track = 0;          // that call read a tracking result (the validity rules of the table apply to the shapes too)
    FeatureParams feat = {0.333, 740.0, 959.0, 1248.0, 0.278636, 1248.0, 0.956129, 0.99702};
    long long* shape_stats = nullptr; // [4]
    hipStream_t shape_stream = nullptr;
    bool shape_ran = false;
    // evaluation against labelled truth (scvod_evaluate_device / scvod_batch_evaluate / scvod_classify_map_device, scvod_eval.hip): one
    // grow-only scratch block and 16 counter words of their own (a grown block must not take an unread result with it); not part of the arena
    Scratch ev;      // stream / ran: the last evaluation (scvod_evaluate_stats waits for it)
    Scratch ev_cls;  // stream / ran of the last scvod_classify_map_device alone: it works in ev's block
    unsigned long long* ev_counters = nullptr;  // [8] evaluation, [8] map classes
    // class scores against labelled truth (scvod_score_classes_device / scvod_batch_score_classes, scvod_classes.hip): a grow-only block
    // and 24 counter words of their own, allocated by the first call
    Scratch cs;  // stream / ran: the last scoring call (scvod_score_classes_stats waits for it)
    unsigned long long* cs_counters = nullptr;
    // object scores (scvod_score_instances_device, scvod_instances.hip): a grow-only block (the global table, the sort's buffers) and 8
    // counter words of their own, allocated by the first call; not part of the arena, not the evaluation's and not the class scores'
    Scratch in;  // stream / ran: the last call (scvod_score_instances_stats waits for it)
    unsigned long long* in_counters = nullptr;
    int in_variant = 0;
    // the truth label of the table's objects (scvod_batch_object_truth, scvod_objtruth.hip): a grow-only block (the spill list, the
    // fallback's regions) and 8 counter words of their own, allocated by the first call; not part of the arena or the table's scratch
    Scratch ot;  // stream / ran: the last call (scvod_batch_object_truth_stats waits for it)
    unsigned long long* ot_counters = nullptr;
    // the objects' vote on the seen-through verdict (scvod_batch_object_visibility, scvod_objvis.hip): a grow-only block (the tiles'
    // accumulators) and 8 counter words of their own, allocated by the first call; not part of the arena or the table's scratch
    Scratch ov;  // stream / ran: the last call (scvod_batch_object_visibility_stats waits for it)
    unsigned long long* ov_counters = nullptr;
    // the ESF descriptor (scvod_esf_device / scvod_batch_object_esf, scvod_objesf.hip): a grow-only block (the workgroups' sample
    // bytes; for the batch form the gathered members and the objects' classes) and 16 counter words of their own, allocated by the
    // first call; not part of the arena or the table's scratch
    Scratch esf;  // stream / ran: the last call (scvod_esf_stats waits for it)
    unsigned long long* esf_counters = nullptr;
    int esf_blocks = 0;  // two workgroups per CU of the device
    hipEvent_t esf_ev = nullptr;  // orders a call behind the last one on another stream: they share the counters and the block
    // the pose refinement against a cloud (scvod_register_device, scvod_register.hip): the state of that unit (its grow-only block, the
    // staged poses and offsets), made by the first call; not part of the arena
    void* reg_state = nullptr;
    // the surface normals of a cloud (scvod_normals_device, scvod_normals.hip): the state of that unit (its grow-only block, the event
    // behind its last call), made by the first call; not part of the arena
    void* nrm_state = nullptr;
    uint64_t types_serial = 0;        // counts the scvod_batch_cluster_types calls of this ctx
    uint64_t obj_lists_types_serial = 0;  // ... at the table call whose lists the scratch holds (the class mask reads the class bytes)
    // the objects linked into tracks (scvod_object_tracks_device / scvod_batch_object_tracks, scvod_tracks.hip): a grow-only block (pose
    // and successor tables, the per-object arrays, the scan's temporary storage) and 8 counter words of their own, allocated by the
    // first call; not part of the arena or the table's scratch
    Scratch trk;  // stream / ran: the last call (scvod_object_tracks_stats waits for it)
    unsigned long long* trk_counters = nullptr;
    std::vector<unsigned char> trk_host;  // the tables as built on the host (the upload is staged from a copy)
    // the tracks' vote on the seen-through verdict (scvod_track_visibility_device, scvod_trackvis.hip): a grow-only block (pose
    // matrices, the per-object and per-track arrays) and 8 counter words of their own, allocated by the first call; not part of the
    // arena and no other stage's scratch
    Scratch tv;  // stream / ran: the last call (scvod_track_visibility_stats waits for it)
    unsigned long long* tv_counters = nullptr;
    std::vector<float> tv_host;  // the pose matrices as built on the host
    // scan stacking (scvod_batch_stack_scans, scvod_stack.hip): the segment and tile tables, one grow-only block of their own allocated
    // by the first call; not part of the arena
    Scratch stk;
    std::vector<unsigned char> stk_host;  // the tables as built on the host (scratch of the call; the upload is staged from a copy)
    // map split by nearest-neighbour hits (scvod_map_split_device, scvod_split.hip): a grow-only block and 8 stats words of their own,
    // allocated by the first call; not part of the arena, not the evaluation's and not the class scores'
    Scratch sp;  // stream / ran: the last split (scvod_map_split_stats waits for it)
    unsigned long long* sp_stats = nullptr;
    // seen-through points (scvod_visibility_device / scvod_batch_visibility, scvod_visibility.hip): a grow-only block (range images,
    // pair / scan / tile tables, the batch form's mask) and 8 counter words of their own, allocated by the first call; not part of the arena
    Scratch vis;  // stream / ran: the last vote (scvod_visibility_stats waits for it)
    unsigned long long* vis_counters = nullptr;
    std::vector<unsigned char> vis_host;  // the tables as built on the host (scratch of the call; the upload is staged from a copy)
    // a cloud against every scan's range image (scvod_cloud_visibility_device, scvod_cloudvis.hip): a grow-only block (matrices, the
    // sort's keys, indices and temporary storage) and 10 counter words of their own, allocated by the first call; not part of the arena
    Scratch cv;  // stream / ran: the last call (scvod_cloud_visibility_stats waits for it)
    unsigned long long* cv_counters = nullptr;
    std::vector<float> cv_host;  // the matrices as built on the host
    std::vector<int32_t> tk_stage;    // host staging of scvod_batch_fetch_track
    // streaming ingest (scvod_sequence_ingest): two device chunk buffers, a copy stream, pinned offsets
    hipStream_t copy_stream = nullptr;
    // the max_name pass (scvod_lastname.hip) runs beside the kernels that follow the clustering, on a stream of its own; whoever
    // needs its result or its scratch waits for ln_done (join_lastname)
    hipStream_t ln_stream = nullptr;
    hipStream_t ln_stream2 = nullptr, ln_stream3 = nullptr;
    hipEvent_t ln_fork = nullptr, ln_done = nullptr, ln_fork2 = nullptr, ln_join2 = nullptr, ln_join3 = nullptr;
    bool ln_pending = false;
    void* ingest_buf[2] = {nullptr, nullptr};
    size_t ingest_cap = 0;  // points per buffer
    hipEvent_t ingest_copied[2] = {nullptr, nullptr}, ingest_done[2] = {nullptr, nullptr};
    int32_t* ingest_off = nullptr;  // pinned
    size_t ingest_off_cap = 0;
    std::vector<uint8_t> tk_stage_dyn;
    // last batch
    bool batch_valid = false;
    std::vector<int32_t> h_scan_off;
    std::vector<int32_t> h_counts;
    bool counts_valid = false;
    bool have_patchwork = false;
    int batch_mode = 0;          // do_patchwork of the last batch: 1 Patchwork+binning, 0 binning only, 2 caller's apri_vec
    bool apri_compact = false;   // PointAPRI records not materialised yet (k_apri_expand on request)
    bool voxels_valid = false;   // the last batch ran the voxel stage in descriptor mode (not VoxelGrid)
    int desc_mode = 0;           // scvod_set_voxel_descriptors: 0 vox_av / vox_cov of a batch on demand (lean voxel stage), 1 eager
    bool desc_valid = false;     // vox_av / vox_cov hold the last batch's values (ensure_descriptors fills them otherwise)
    bool int_valid = true;       // apri_int holds the last batch's intensities (a lean emission leaves them out: ensure_intensities)
    bool lists_valid = true;     // ground_idx / nonground_idx / rejected_src hold the last batch's lists (a lean emission leaves them out: ensure_lists)
    bool clusters_valid = false;
    bool clustered_this_batch = false;       // the batch's pt_mapcls bytes carry car / dynamic marks of an earlier clustering (cleared before the next one)
    bool types_valid = false;
    hipStream_t last_stream = nullptr;
    // host staging for scvod_scan_result
    Scratch nn[6];  // scvod_nn_search scratch; `ran` stays false: the host forms synchronise before they return
    void* stage = nullptr;       // pinned host block holding the arrays of the last scvod_scan_result
    size_t stage_bytes = 0;
    // timing
    bool timing = false;
    std::vector<TimingEntry> tim;
    size_t tim_used = 0;
    std::string err;
};

namespace {

int fail(scvod_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess) return fail(ctx, SCVOD_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {
    unsigned char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t count) {
        off = align_up(off, 256);
        T* p = base ? (T*)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

void carve(scvod_ctx* c, unsigned char* base, size_t* total) {
    const size_t N = (size_t)c->cap_pts, B = (size_t)c->cap_scans;
    Carver k{base};
    Arena& A = c->A;
    c->d_scan_off = k.take<int32_t>(B + 1);
    A.pid = k.take<int16_t>(N);
    A.keys = k.take<uint64_t>(N);
    A.seg = k.take<uint32_t>(N);
    A.ln_scratch = A.seg;  // (scvod_batch_cluster decides it again)
    A.sorted_xyz = k.take<Xyz>(N + 8);
    A.sorted_idx = k.take<uint32_t>(N);
    A.zkey = k.take<uint32_t>(N);
    A.fit_thd = k.take<float>(B * kMaxPatches);
    A.order = k.take<int4>(B * kMaxPatches);
    A.order_hist = k.take<int32_t>(64);
    A.order_cursor = k.take<int32_t>(64);
    A.order_off = k.take<int32_t>(65);
    A.patch_count = k.take<int32_t>(B * kMaxPatches);
    A.patch_cursor = k.take<int32_t>(B * kMaxPatches);
    A.patch_off = k.take<int32_t>(B * (kMaxPatches + 1));
    A.patch_rec = k.take<PatchRec>(B * kMaxPatches);
    A.planes = k.take<scvod_patch_plane>(B * kMaxPatches);
    A.emit_off = k.take<int32_t>(B * kMaxPatches * 4);
    A.cls = k.take<uint8_t>(N);
    A.ground_idx = k.take<int32_t>(N);
    A.nonground_idx = k.take<int32_t>(N);
    A.apri = c->d_apri;  // (side buffer: ensure_side; nullptr until something asks for PointAPRI records)
    A.apri_src = k.take<int32_t>(N);
    A.apri_key = k.take<int32_t>(N);
    A.apri_int = k.take<float>(N);
    A.apri_idx3 = k.take<int32_t>(N);
    A.rejected_src = k.take<int32_t>(N);
    A.counts = k.take<int32_t>(B * 8);
    A.scan_irr = k.take<int32_t>(B);
    A.irr_list = k.take<int32_t>(B * (kIrrListCap + 1));
    A.cc_perm = k.take<int32_t>(B);
    A.vb_count = k.take<int32_t>(B * kMaxBuckets);
    A.vb_off = k.take<int32_t>(B * (kMaxBuckets + 1));
    A.vb_nvox = k.take<int32_t>(B * kMaxBuckets);
    A.vox_off = k.take<int32_t>(B * (kMaxBuckets + 1));
    A.vorder = k.take<int4>(B * kMaxBuckets);
    A.vorder_hist = k.take<int32_t>(64);
    A.vorder_cursor = k.take<int32_t>(64);
    A.vorder_off = k.take<int32_t>(65);
    A.vkeys = k.take<uint64_t>(N);
    A.tmp_vox_key = k.take<int32_t>(N);
    A.tmp_vox_begin = k.take<int32_t>(N);
    A.tmp_vox_av = k.take<float>(N);
    A.tmp_vox_cov = k.take<float>(N);
    A.vox_key = k.take<int32_t>(N);
    A.vox_pt_begin = k.take<int32_t>(N + B);
    A.vox_pts = k.take<int32_t>(N);
    A.vox_av = k.take<float>(N);
    A.vox_cov = k.take<float>(N);
    A.cc_stats = k.take<int32_t>(8);
    A.cc_again = k.take<int32_t>(B + 1);
    A.cc_help = k.take<int32_t>(kCcHelpWords);
    A.cc_help_blocks = 0;
    A.cc_help_blocks_wanted = 1;
    A.cc_exact_max = 0x3fffffff;  // (round 6: exact whatever the component's size is the default -- the passes are shared with helper blocks, k_cc_exact)
    A.cc_plain_rule = 1;
    A.cc_parent = k.take<int32_t>(N);
    A.cc_touched = k.take<uint8_t>(N);
    A.pt_voxel = k.take<int32_t>(N);
    A.pt_cluster = k.take<int32_t>(N);
    A.cl_bbox = k.take<uint32_t>(7 * N + 64);
    A.cl_count = k.take<int32_t>(N);
    A.pt_type = k.take<uint8_t>(N);
    A.cc_last = k.take<int32_t>(B * 4);
    A.cc_redo = k.take<int32_t>(4 * (B + 1));
    A.ln_state = k.take<int32_t>(B * 2048);
    A.ln_stats = k.take<int32_t>(4);
    A.ln_prof = k.take<int32_t>(B * 8);
    A.ln_prof2 = k.take<int32_t>(B * 8);
    A.vg_par = k.take<int32_t>(B * 16);
    A.vg_range = k.take<int32_t>(2);  // [0] largest cell-index range of the batch, [1] bin shift of the bucket table
    A.vg_outoff = k.take<int32_t>(B + 1);
    c->d_vb_lut = k.take<uint16_t>(B * kVgLutBins);
    A.vb_lut = nullptr;  // hot path: uniform key ranges (DevParams::vb_shift)
    A.vb_lut_shift = nullptr;
    A.vg_labels = nullptr;
    A.vg_max_intensity = 1.f;
    c->t_hit = k.take<int32_t>(N);
    c->t_work = k.take<uint64_t>(N);
    c->t_uniq = k.take<int32_t>(N);
    c->t_begin = k.take<int32_t>(N + 1);
    c->t_pair = k.take<int32_t>(N);
    c->t_pairpt = k.take<int32_t>(B + 1);
    c->t_count = k.take<int32_t>(N);
    c->t_T = k.take<float>(12 * (B + 1));
    // sequence differencing on the device: the per-pair scratch above is never in use at the same time
    A.tk_hit = c->t_hit;
    A.tk_uniq = c->t_uniq;
    A.tk_nuniq = c->t_count;
    A.tk_cursor = c->t_pair;
    A.tk_mbegin = k.take<int32_t>(N + 1);  // (published by the clustering: not shared with the one-shot probe's scratch)
    A.vox_track = k.take<int4>(N);
    A.vox_rep = k.take<int32_t>(N);
    A.tk_crep = k.take<int32_t>(N);
    A.tk_prep = k.take<int32_t>(N);
    A.cl_state = k.take<int8_t>(N);
    A.tk_members = k.take<int32_t>(N);
    A.tk_pairs = k.take<int2>(N);
    A.tk_npairs = k.take<int32_t>(N);
    A.tk_clusters = k.take<int32_t>(N);
    A.tk_scan = k.take<int32_t>(B * 4);
    A.pt_dyn = k.take<uint8_t>(N);
    A.pt_mapcls = k.take<uint8_t>(N);
    c->d_next_scan = k.take<int32_t>(B);
    c->d_ext = k.take<const int4*>(B);
    c->d_chain_scans = k.take<int32_t>(B);
    c->d_chain_walkers = k.take<ChainWalker>(B);
    c->d_chain_fw = k.take<int32_t>(B + 1);
    c->d_chain_stats = k.take<int32_t>(8);
    c->d_step_ticks = k.take<int32_t>(B + 1);
    c->d_chain_cmp = k.take<int32_t>(4);
    c->d_ext_state = k.take<const unsigned char*>(B);
    *total = align_up(k.off, 256);
}

void build_dev_params(scvod_ctx* c) {
    const scvod_params& p = c->params;
    const scvod_pw_params& w = c->pw;
    DevParams& D = c->dev;
    memset(&D, 0, sizeof(D));
    BinParams& b = D.bin;
    b.min_dis = p.min_dis;
    b.max_dis = p.max_dis;
    b.min_angle = p.min_angle;
    b.max_angle = p.max_angle;
    b.min_azimuth = p.min_azimuth;
    b.max_azimuth = p.max_azimuth;
    b.range_res = p.range_res;
    b.sector_res = p.sector_res;
    b.azimuth_res = p.azimuth_res;
    scvod_grid_dims(&p, &b.range_num, &b.sector_num, &b.azimuth_num, &b.bin_num);
    D.keep = keep_fast_of(b);
    D.binfast = bin_fast_of(b);
    CzmParams& z = D.czm;
    z.min_range = w.min_range;
    z.max_range = w.max_range;
    // patchwork.h:83-94
    const double z2 = (7 * w.min_range + w.max_range) / 8.0;
    const double z3 = (3 * w.min_range + w.max_range) / 4.0;
    const double z4 = (w.min_range + w.max_range) / 2.0;
    z.zone_min[0] = w.min_range;
    z.zone_min[1] = z2;
    z.zone_min[2] = z3;
    z.zone_min[3] = z4;
    z.ring_size[0] = (z2 - w.min_range) / w.num_rings_each_zone[0];
    z.ring_size[1] = (z3 - z2) / w.num_rings_each_zone[1];
    z.ring_size[2] = (z4 - z3) / w.num_rings_each_zone[2];
    z.ring_size[3] = (w.max_range - z4) / w.num_rings_each_zone[3];
    int base = 0;
    for (int k = 0; k < 4; ++k) {
        z.sector_size[k] = 2 * M_PI / w.num_sectors_each_zone[k];
        z.num_rings[k] = w.num_rings_each_zone[k];
        z.num_sectors[k] = w.num_sectors_each_zone[k];
        z.patch_base[k] = base;
        base += w.num_rings_each_zone[k] * w.num_sectors_each_zone[k];
        z.elevation_thr[k] = w.elevation_thr[k];
        z.flatness_thr[k] = w.flatness_thr[k];
    }
    z.num_patches = base;
    const double sensor_height = (double)p.sensor_height;  // set_sensor(const double&), ssc.cpp:93
    z.z_cut = -1.8 * sensor_height;
    z.seed_margin_z = w.adaptive_seed_selection_margin * sensor_height;
    z.th_seeds = w.th_seeds;
    z.th_dist = w.th_dist;
    z.uprightness_thr = w.uprightness_thr;
    z.num_iter = w.num_iter;
    z.num_lpr = w.num_lpr;
    z.num_min_pts = w.num_min_pts;
    z.num_rings_of_interest = w.num_rings_of_interest;
    czm_finalize(z);
    D.n_patches = base;
    D.max_z = p.max_z;
    D.min_z = p.min_z;
    D.car_square = p.car_square;
    D.to_be_class = p.toBeClass;
    // voxel buckets: keys of filtered points lie in [-(R*S+S+1), bin_num)
    D.key_off = (int64_t)b.range_num * b.sector_num + b.sector_num + 1;
    int64_t range = (int64_t)b.bin_num + D.key_off + 1;
    int shift = 12;
    while (((range >> shift) + 1) > kMaxBuckets) ++shift;
    D.vb_shift = shift;
    D.n_buckets = (int32_t)((range >> shift) + 1);
}

void timer_hook(void* user, const char* name, int begin) {
    scvod_ctx* c = (scvod_ctx*)user;
    static const bool trace = getenv("SCVOD_TRACE") != nullptr;
    if (trace) {  // debugging aid: name every launch and synchronise after it
        if (!begin) {
            hipError_t e = hipStreamSynchronize(c->last_stream);
            fprintf(stderr, "[scvod] %s done: %s\n", name, hipGetErrorString(e));
        } else {
            fprintf(stderr, "[scvod] %s ...\n", name);
        }
        fflush(stderr);
    }
    if (!c->timing) return;
    hipStream_t st = c->last_stream;
    if (begin) {
        if (c->tim_used == c->tim.size()) {
            TimingEntry t;
            t.name = name;
            hipEventCreate(&t.e0);
            hipEventCreate(&t.e1);
            c->tim.push_back(t);
        }
        c->tim[c->tim_used].name = name;
        hipEventRecord(c->tim[c->tim_used].e0, st);
    } else {
        hipEventRecord(c->tim[c->tim_used].e1, st);
        c->tim_used++;
    }
}

// Makes `st` wait for the max_name pass of the last clustering (if one is still in flight).
static void join_lastname(scvod_ctx* c, hipStream_t st) {
    if (!c->ln_pending) return;
    hipStreamWaitEvent(st, c->ln_done, 0);
    c->ln_pending = false;
}

// Buffers that only the per-scan host API, the one-shot probe, the VoxelGrid run and a fetch of PointAPRI records touch: 80 of
// what used to be 318 bytes per point of the arena, allocated on first use (round 5: a sequence shard that stays in the batch
// API never pays for them -- 26 GB of the seq-05 job's 104).
enum SideBuf { kSideIn = 1, kSideTpts = 2, kSideLabels = 4, kSideApri = 8 };
int ensure_side(scvod_ctx* c, int which) {
    const size_t N = (size_t)c->cap_pts;
    auto need = [&](void** p, size_t bytes) -> int {
        if (*p) return SCVOD_OK;
        HIPCHK(c, hipMalloc(p, bytes));
        c->side_bytes += bytes;
        return SCVOD_OK;
    };
    int rc = SCVOD_OK;
    if ((which & kSideIn) && (rc = need((void**)&c->d_in, sizeof(float4) * N))) return rc;
    if ((which & kSideTpts) && (rc = need((void**)&c->t_pts, sizeof(float4) * N))) return rc;
    if ((which & kSideLabels) && (rc = need((void**)&c->d_labels, sizeof(uint32_t) * N))) return rc;
    if ((which & kSideApri) && (rc = need((void**)&c->d_apri, sizeof(scvod_apri) * N))) return rc;
    c->A.apri = c->d_apri;
    return rc;
}

// scratch of the intensity merge: one allocation carved like the arena, made the first time a clustering merges
int ensure_merge(scvod_ctx* c) {
    if (c->im_buf) return SCVOD_OK;
    const size_t N = (size_t)c->cap_pts, B = (size_t)c->cap_scans;
    for (int pass = 0; pass < 2; ++pass) {
        Carver k{(unsigned char*)c->im_buf};
        MergeJob& M = c->im;
        M.vlab = k.take<int32_t>(N);
        M.key0 = k.take<int32_t>(N);
        M.nxt = k.take<int32_t>(N);
        M.own = k.take<uint8_t>(N);
        M.fz = k.take<uint8_t>(N);
        M.qv = k.take<int32_t>(N);
        M.qk = k.take<int32_t>(N);
        M.box = k.take<uint32_t>(7 * N);
        M.pair = k.take<uint64_t>(kImPairsPerPt * N + kImPairsPerScan * B);
        M.cand = k.take<uint64_t>(N);
        M.pt_merged = k.take<int32_t>(N);
        M.stats = k.take<int32_t>(8);
        if (pass == 0) {
            c->im_bytes = align_up(k.off, 256);
            HIPCHK(c, hipMalloc(&c->im_buf, c->im_bytes));
            c->side_bytes += c->im_bytes;
        }
    }
    return SCVOD_OK;
}

// the chunks of a batch of B scans for the chunked opt-in stages: f(s0, s1) for consecutive runs [s0, s1) of at most max_scans scans
// and at most max_pts points (more points only when a single scan is larger)
template <typename F>
void scan_chunks(const std::vector<int32_t>& off, int B, int max_scans, int64_t max_pts, F f) {
    for (int s0 = 0; s0 < B;) {
        int s1 = s0 + 1;
        while (s1 < B && s1 - s0 < max_scans && (int64_t)off[s1 + 1] - off[s0] <= max_pts) ++s1;
        f(s0, s1);
        s0 = s1;
    }
}

// scratch of the region growing for chunks of up to `chunk` points, and its outputs over the ctx's capacity: allocated on first use
constexpr int64_t kRgChunkPts = 1 << 23;  // points of the scans of one chunk
constexpr int kRgChunkScans = 65535;      // (the scans of a chunk are a launch grid's y)
int ensure_rgrow(scvod_ctx* c, int64_t chunk) {
    const size_t N = (size_t)c->cap_pts;
    RgJob& J = c->rg;
    if (!c->rg_out) {
        Carver k{nullptr};
        for (int pass = 0; pass < 2; ++pass) {
            k = Carver{(unsigned char*)c->rg_out};
            J.cls = k.take<uint8_t>(N);
            J.out_nc = k.take<float4>(N);
            J.out_seg = k.take<int32_t>(N);
            J.stats = k.take<int32_t>(8);
            J.cnt = k.take<int32_t>(2);
            if (pass == 0) {
                c->rg_out_bytes = align_up(k.off, 256);
                HIPCHK(c, hipMalloc(&c->rg_out, c->rg_out_bytes));
                c->side_bytes += c->rg_out_bytes;
            }
        }
        HIPCHK(c, hipEventCreateWithFlags(&c->rg_ev, hipEventDisableTiming));
    }
    if (c->rg_cap >= chunk) return SCVOD_OK;
    if (c->rg_buf) {
        HIPCHK(c, hipStreamSynchronize(c->last_stream));
        HIPCHK(c, hipFree(c->rg_buf));
        HIPCHK(c, hipFree(c->rg_sort_tmp));
        c->side_bytes -= c->rg_buf_bytes + c->rg_sort_bytes;
        c->rg_buf = c->rg_sort_tmp = nullptr;
    }
    const size_t C = (size_t)chunk;
    for (int pass = 0; pass < 2; ++pass) {
        Carver k{(unsigned char*)c->rg_buf};
        J.bmin = k.take<uint32_t>(3 * C);
        J.bmax = k.take<uint32_t>(3 * C);
        J.bcnt = k.take<int32_t>(C);
        J.key_in = k.take<uint64_t>(C);
        J.key_out = k.take<uint64_t>(C);
        J.cl = k.take<int2>(C);
        J.cl_name = k.take<int32_t>(C);
        J.grid = k.take<float4>(2 * C);
        J.cell = k.take<int32_t>(3 * C);
        J.pcell = k.take<int32_t>(C);
        J.cell_pts = k.take<int32_t>(C);
        J.pos_cl = k.take<int32_t>(C);
        J.pl = k.take<int2>(C);
        J.cxyz = k.take<float4>(C);
        J.nbr = k.take<int32_t>(16 * C);
        J.nrm = k.take<float4>(C);
        J.emask = k.take<uint16_t>(C);
        J.lab = k.take<uint64_t>(C);
        J.segc = k.take<int32_t>(C);
        J.tail = k.take<int32_t>(C);
        if (pass == 0) {
            c->rg_buf_bytes = align_up(k.off, 256);
            HIPCHK(c, hipMalloc(&c->rg_buf, c->rg_buf_bytes));
            c->rg_sort_bytes = rg_sort_bytes((int)chunk);
            HIPCHK(c, hipMalloc(&c->rg_sort_tmp, c->rg_sort_bytes));
            c->side_bytes += c->rg_buf_bytes + c->rg_sort_bytes;
        }
    }
    c->rg_cap = chunk;
    return SCVOD_OK;
}

// the region growing over the batch, chunk by chunk of scans, on stream st
int run_rgrow(scvod_ctx* c, hipStream_t st) {
    const int B = c->A.n_scans;
    const std::vector<int32_t>& off = c->h_scan_off;
    int64_t need = 1;
    scan_chunks(off, B, kRgChunkScans, kRgChunkPts, [&](int s0, int s1) { need = std::max(need, (int64_t)off[s1] - off[s0]); });
    int rc = ensure_rgrow(c, need);
    if (rc) return rc;
    RgJob& J = c->rg;
    J.k = c->rg_k;
    J.min_seg = c->rg_min_seg;
    J.max_seg = 1000000;  // setMaxClusterSize (ssc.cpp:808)
    J.cos_t = c->rg_cos;
    J.curv_thr = c->rg_curv;
    J.frac = c->rg_frac;
    J.from_apri = c->batch_mode == 2 ? 1 : 0;
    HIPCHK(c, hipMemsetAsync(J.stats, 0, 8 * sizeof(int32_t), st));
    scan_chunks(off, B, kRgChunkScans, kRgChunkPts, [&](int s0, int s1) {
        J.s0 = s0;
        J.ns = s1 - s0;
        J.off0 = off[s0];
        launch_rgrow(c->dev, c->A, J, (int)(off[s1] - off[s0]), c->rg_sort_tmp, c->rg_sort_bytes, st, timer_hook, c);
    });
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

// scratch of the intensity calibration for chunks of up to `chunk` points: allocated on first use
constexpr int64_t kCalChunkPts = 1 << 22;  // points of the scans of one chunk
int ensure_calib(scvod_ctx* c, int64_t chunk) {
    if (c->cal_cap >= chunk) return SCVOD_OK;
    CalJob& J = c->cal;
    if (c->cal_buf) {
        HIPCHK(c, hipStreamSynchronize(c->last_stream));
        HIPCHK(c, hipFree(c->cal_buf));
        c->side_bytes -= c->cal_buf_bytes;
        c->cal_buf = nullptr;
    }
    const size_t C = (size_t)chunk;
    for (int pass = 0; pass < 2; ++pass) {
        Carver k{(unsigned char*)c->cal_buf};
        J.sxyz = k.take<float4>(C);
        J.pcell = k.take<int32_t>(C);
        J.cell = k.take<int32_t>(3 * C + 4 * (size_t)kCalChunkScans);
        J.slot = k.take<int32_t>(C);
        J.grid = k.take<float4>(2 * (size_t)kCalChunkScans);
        J.stats = k.take<int32_t>(8);
        J.cand = k.take<unsigned long long>(1);
        if (pass == 0) {
            c->cal_buf_bytes = align_up(k.off, 256);
            HIPCHK(c, hipMalloc(&c->cal_buf, c->cal_buf_bytes));
            c->side_bytes += c->cal_buf_bytes;
        }
    }
    c->cal_cap = chunk;
    return SCVOD_OK;
}

// the intensity calibration over the batch, chunk by chunk of scans, on stream st (between k_emit and the voxel stage)
int run_calib(scvod_ctx* c, hipStream_t st) {
    const int B = c->A.n_scans;
    const std::vector<int32_t>& off = c->h_scan_off;
    int64_t need = 1;
    scan_chunks(off, B, kCalChunkScans, kCalChunkPts, [&](int s0, int s1) { need = std::max(need, (int64_t)off[s1] - off[s0]); });
    int rc = ensure_calib(c, need);
    if (rc) return rc;
    CalJob J = c->cal;
    J.k = c->cal_k;
    J.max_int = c->cal_max;
    J.write_apri = 1;
    J.out_int = nullptr;
    J.out_nc = nullptr;
    static const bool force = getenv("SCVOD_CALIB_FORCE_FALLBACK") != nullptr;  // (development: tools/intensity_calibration_cost.py)
    J.force_fallback = force ? 1 : 0;
    HIPCHK(c, hipMemsetAsync(J.stats, 0, 8 * sizeof(int32_t), st));
    HIPCHK(c, hipMemsetAsync(J.cand, 0, sizeof(unsigned long long), st));
    scan_chunks(off, B, kCalChunkScans, kCalChunkPts, [&](int s0, int s1) {
        J.s0 = s0;
        J.ns = s1 - s0;
        J.off0 = off[s0];
        launch_calib(c->A, J, (int)(off[s1] - off[s0]), st, timer_hook, c);
    });
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

// everything after the clustering reads the partition through A.pt_cluster: the fused one after a merged clustering.  A new batch
// or clustering starts from the arena's own array again.
void unmerge_view(scvod_ctx* c) {
    c->rg_done = false;  // (the region growing's outputs belong to the clustering they were computed on)
    if (c->pt_cluster_own) c->A.pt_cluster = c->pt_cluster_own;
    c->merged = false;
    c->im_overflow = -1;
}

// a merged clustering whose neighbour pairs outgrew their scratch left some scans unmerged: every reader of the result fails
int merge_check(scvod_ctx* c) {
    if (!c->merged) return SCVOD_OK;
    if (c->im_overflow < 0) {
        HIPCHK(c, hipStreamSynchronize(c->last_stream));
        int32_t st[8];
        HIPCHK(c, hipMemcpy(st, c->im.stats, sizeof(st), hipMemcpyDeviceToHost));
        c->im_overflow = st[4];
    }
    if (c->im_overflow > 0)
        return fail(c, SCVOD_ERR_CAPACITY, "intensity merge: the neighbour pairs of %d scans outgrew their scratch (%d per point + %d per scan)", c->im_overflow, kImPairsPerPt, kImPairsPerScan);
    return SCVOD_OK;
}

// lean_ok: a batch entry, whose descriptors may wait for their first reader (ensure_descriptors); the per-scan API hands them to the
// host at once and keeps the fused form
int run_batch(scvod_ctx* c, const void* d_xyzi, const int32_t* h_off, int32_t n_scans, hipStream_t st,
              int do_patchwork, int apply_filter, int do_voxels, int sync, bool off_pinned = false, bool lean_ok = false) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_scans <= 0 || !h_off || (!d_xyzi && do_patchwork != 2)) return fail(c, SCVOD_ERR_INVALID, "empty batch");
    unmerge_view(c);
    if (n_scans > c->cap_scans) return fail(c, SCVOD_ERR_CAPACITY, "n_scans %d > capacity %d", n_scans, c->cap_scans);
    int64_t total = (int64_t)h_off[n_scans] - h_off[0];
    if (h_off[0] != 0) return fail(c, SCVOD_ERR_INVALID, "scan_offsets[0] must be 0");
    if (total > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "%lld points > capacity %lld", (long long)total, (long long)c->cap_pts);
    int32_t mx = 0;
    for (int s = 0; s < n_scans; ++s) {
        int32_t n = h_off[s + 1] - h_off[s];
        if (n < 0) return fail(c, SCVOD_ERR_INVALID, "scan_offsets not monotone");
        if (n > mx) mx = n;
    }
    if (mx > SCVOD_MAX_SCAN_POINTS)
        return fail(c, SCVOD_ERR_CAPACITY, "scan of %d points > SCVOD_MAX_SCAN_POINTS (%d)", mx, SCVOD_MAX_SCAN_POINTS);
    HIPCHK(c, hipSetDevice(c->device));
    if (!st) st = c->stream;
    c->last_stream = st;
    join_lastname(c, st);
    c->h_scan_off.assign(h_off, h_off + n_scans + 1);
    if (do_patchwork != 1) {  // (binning without Patchwork writes the PointAPRI records, a caller's apri_vec lives in them)
        const int rc_side = ensure_side(c, kSideApri);
        if (rc_side) return rc_side;
    }
    // (a caller-pinned offset table is read by the copy engine directly: nothing to wait for on the host)
    HIPCHK(c, hipMemcpyAsync(c->d_scan_off, off_pinned ? h_off : c->h_scan_off.data(), sizeof(int32_t) * (n_scans + 1), hipMemcpyHostToDevice, st));
    c->A.pts = (const float4*)d_xyzi;
    c->A.scan_off = c->d_scan_off;
    c->A.n_scans = n_scans;
    c->A.max_scan_pts = mx;
    c->A.total_pts = total;
    {   // 32-bit voxel sort keys when a bucket-relative key and a scan-local index fit together (filtered keys never leave the grid)
        int ib = 1;
        while ((1 << ib) < mx) ++ib;
        c->A.vx_idx_bits = ib;
        c->A.vx_k32 = (do_patchwork != 3 && apply_filter && c->dev.vb_shift + ib <= 32) ? 1 : 0;
    }
    c->tim_used = 0;
    c->batch_valid = false;
    c->counts_valid = false;
    c->voxels_valid = false;
    c->desc_valid = false;
    c->clusters_valid = false;
    c->types_valid = false;
    c->track_valid = false;
    c->tables_valid = false;
    // a ctx with the intensity merge on reads every descriptor in its clustering: it keeps the fused form (lean + on demand measured
    // 0.7 ms slower for it, profiles/lazy_voxel_descriptors_cost.md; SCVOD_VOX_LEAN_MERGE: development, that measurement)
    static const bool lean_merge = getenv("SCVOD_VOX_LEAN_MERGE") != nullptr;
    const int lean = (lean_ok && do_voxels && do_patchwork != 3 && c->desc_mode == 0 && (c->im_iterations == 0 || lean_merge)) ? 1 : 0;
    // the lean emission (k_emit<true>: no point gather, no apri_int) goes with the lean voxel stage, whose kernels never read an
    // intensity; the calibration reads and patches apri_int right behind the emission, and a grid beyond the packed triple's limits
    // cannot have its voxel key recomputed from it: both keep the gather form
    const int lean_emit = (lean && do_patchwork == 1 && !c->cal_on && idx3_roundtrip_ok(c->dev.bin)) ? 1 : 0;
    // marks per input point for the static map (car-cluster member / dynamic / list marks): clean for every new batch
    if (mx > 0 && do_patchwork != 2 && do_patchwork != 3) HIPCHK(c, hipMemsetAsync(c->A.pt_mapcls, 0, (size_t)total, st));
    c->clustered_this_batch = false;
    c->cal_done = false;
    if (mx > 0 && c->cal_on && do_patchwork == 1) {  // Patchwork + binning, the calibration of apri_int, then the voxel stage on its own
        launch_process(c->dev, c->A, st, 1, apply_filter, 0, timer_hook, c);
        const int rc_cal = run_calib(c, st);
        if (rc_cal) return rc_cal;
        if (do_voxels) launch_process(c->dev, c->A, st, 4, apply_filter, 1, timer_hook, c, lean);
    } else if (mx > 0) {
        launch_process(c->dev, c->A, st, do_patchwork, apply_filter, do_voxels, timer_hook, c, lean, lean_emit);
    }
    c->cal_done = c->cal_on && do_patchwork == 1;  // (a batch of empty scans is a calibrated batch of no points)
    HIPCHK(c, hipGetLastError());
    if (mx == 0) {  // every scan empty: no kernel runs (neither here nor in the clustering / tracking launches): clean per-scan words
        HIPCHK(c, hipMemsetAsync(c->A.counts, 0, sizeof(int32_t) * 8 * n_scans, st));
        HIPCHK(c, hipMemsetAsync(c->A.tk_scan, 0, sizeof(int32_t) * 4 * n_scans, st));
    }
    c->batch_valid = true;
    c->voxels_valid = (do_voxels != 0);
    c->desc_valid = (do_voxels != 0) && !lean;  // (every process call decides it again: a lean batch's descriptors are not there yet)
    c->int_valid = !(lean_emit && mx > 0);
    c->lists_valid = !(lean_emit && mx > 0);  // (every process call decides it again, as int_valid)
    c->have_patchwork = (do_patchwork == 1);
    c->batch_mode = do_patchwork;
    c->apri_compact = (do_patchwork == 1);
    if (sync) HIPCHK(c, hipStreamSynchronize(st));
    return SCVOD_OK;
}

int ensure_counts(scvod_ctx* c) {
    if (!c->batch_valid) return fail(c, SCVOD_ERR_STATE, "no batch has been run");
    if (c->counts_valid) return SCVOD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    c->h_counts.resize((size_t)c->A.n_scans * 8);
    HIPCHK(c, hipMemcpy(c->h_counts.data(), c->A.counts, sizeof(int32_t) * c->h_counts.size(), hipMemcpyDeviceToHost));
    c->counts_valid = true;
    return SCVOD_OK;
}

// Every reader of apri_int comes through here first: a lean emission left it unwritten, k_apri_intensity fills it for the whole batch
// on stream st at the first request.  Its inputs (the input cloud, apri_src, counts) outlive the batch's chain.  Today's readers:
// k_vx_descriptors (below).  The fused voxel tiers, the calibration and its k_cal_apri run only in a ctx that emitted eagerly; the
// expansion to PointAPRI records reads the input cloud itself.
int ensure_intensities(scvod_ctx* c, hipStream_t st) {
    if (c->int_valid) return SCVOD_OK;
    launch_apri_intensity(c->A, st, timer_hook, c);
    HIPCHK(c, hipGetLastError());
    c->int_valid = true;
    return SCVOD_OK;
}

// Every reader of vox_av / vox_cov comes through here first: a lean voxel stage left them unwritten, k_vx_descriptors fills them for the
// whole batch on stream st -- ordered behind the batch's own kernels there -- at the first request.  Its inputs (vox_pt_begin, vox_pts,
// apri_int) are written by the voxel stage and its predecessors only; no later stage uses them as scratch.
int ensure_descriptors(scvod_ctx* c, hipStream_t st) {
    if (!c->voxels_valid || c->desc_valid) return SCVOD_OK;
    if (int rc_int = ensure_intensities(c, st)) return rc_int;
    launch_vox_descriptors(c->A, 0, c->A.n_scans, st, timer_hook, c);
    HIPCHK(c, hipGetLastError());
    c->desc_valid = true;
    return SCVOD_OK;
}

// Every reader of ground_idx / nonground_idx / rejected_src comes through here first: a lean emission left them unwritten, k_emit_lists
// fills the three for the whole batch on stream st -- ordered behind the batch's own kernels there -- at the first request.  Today's
// readers: fetch_scan (the lists and, through k_cls_from_lists, cls), the label / class kernels of scvod_export.hip, k_map_mark_lists
// (scvod__ctx_ensure_lists) and the calibration, whose ctx emits eagerly anyway.  Its inputs (order, order_off, patch_rec, emit_off, seg)
// are written by the Patchwork kernels only; the one stage that takes scratch from them, the max_name pass with its tables in the arena,
// takes the scan's slice of ground_idx instead while the lists are pending (Arena::ln_scratch): this call waits for that pass and
// then rewrites the slice wholly.
int ensure_lists(scvod_ctx* c, hipStream_t st) {
    if (c->lists_valid) return SCVOD_OK;
    if (c->ln_done) HIPCHK(c, hipStreamWaitEvent(st, c->ln_done, 0));  // (whichever stream joined the pass before: this one reads after it too)
    launch_emit_lists(c->A, st, timer_hook, c);
    HIPCHK(c, hipGetLastError());
    c->lists_valid = true;
    return SCVOD_OK;
}

int fetch_scan(scvod_ctx* c, int32_t s, scvod_scan_result* out) {
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t* k = &c->h_counts[(size_t)s * 8];
    const size_t base = (size_t)c->h_scan_off[s];
    memset(out, 0, sizeof(*out));
    out->n_points = k[0];
    out->n_ground = k[1];
    out->n_nonground = k[2];
    out->n_dropped = k[3];
    out->n_apri = k[4];
    out->n_rejected = k[5];
    out->n_voxels = k[6];
    out->n_patches = k[7];
    if (c->apri_compact && k[4] > 0) {
        const int rc_side = ensure_side(c, kSideApri);
        if (rc_side) return rc_side;
    }
    const Arena& A = c->A;
    hipStream_t st = c->last_stream;
    if (int rc_desc = ensure_descriptors(c, st)) return rc_desc;
    if (int rc_lists = ensure_lists(c, st)) return rc_lists;
    if (c->have_patchwork) launch_cls(A, s, base, k[0], st);
    if (c->apri_compact && k[4] > 0) launch_apri_expand(c->dev, A, s, 1, k[4], st);  // PointAPRI records of this scan only
    if (c->apri_compact && c->cal_done) launch_calib_apri(A, s, k[4], st);             // ... with the calibrated intensity (a second small
                                                                                       //     kernel per fetch: k_apri_expand stays as it was)
    HIPCHK(c, hipGetLastError());
    // one pinned staging block, twelve asynchronous copies, one synchronisation (the pointers handed out live in it)
    struct Part {
        const void* src;
        size_t bytes;
        size_t at;
    };
    const size_t n_cls = c->have_patchwork ? (size_t)k[0] : 0;
    Part parts[12] = {{A.cls + base, n_cls, 0},
                      {A.ground_idx + base, 4 * (size_t)k[1], 0},
                      {A.nonground_idx + base, 4 * (size_t)k[2], 0},
                      {A.planes + (size_t)s * kMaxPatches, sizeof(scvod_patch_plane) * (size_t)k[7], 0},
                      {A.apri ? A.apri + base : nullptr, A.apri ? sizeof(scvod_apri) * (size_t)k[4] : 0, 0},
                      {A.apri_src + base, 4 * (size_t)k[4], 0},
                      {A.rejected_src + base, 4 * (size_t)k[5], 0},
                      {A.vox_key + base, 4 * (size_t)k[6], 0},
                      {A.vox_pt_begin + base + s, 4 * ((size_t)k[6] + 1), 0},
                      {A.vox_pts + base, 4 * (size_t)k[4], 0},
                      {A.vox_av + base, 4 * (size_t)k[6], 0},
                      {A.vox_cov + base, 4 * (size_t)k[6], 0}};
    size_t need = 0;
    for (Part& p : parts) {
        p.at = need;
        need += (p.bytes + 63) & ~(size_t)63;
    }
    need += 64;
    if (need > c->stage_bytes) {
        if (c->stage) hipHostFree(c->stage);
        c->stage = nullptr;
        c->stage_bytes = 0;
        HIPCHK(c, hipHostMalloc(&c->stage, need + need / 4, hipHostMallocDefault));
        c->stage_bytes = need + need / 4;
    }
    char* h = (char*)c->stage;
    for (const Part& p : parts)
        if (p.bytes) HIPCHK(c, hipMemcpyAsync(h + p.at, p.src, p.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (k[6] == 0) *(int32_t*)(h + parts[8].at) = 0;
    out->cls = (const uint8_t*)(h + parts[0].at);
    out->ground_idx = (const int32_t*)(h + parts[1].at);
    out->nonground_idx = (const int32_t*)(h + parts[2].at);
    out->planes = (const scvod_patch_plane*)(h + parts[3].at);
    out->apri = (const scvod_apri*)(h + parts[4].at);
    out->apri_src = (const int32_t*)(h + parts[5].at);
    out->rejected_src = (const int32_t*)(h + parts[6].at);
    out->vox_key = (const int32_t*)(h + parts[7].at);
    out->vox_pt_begin = (const int32_t*)(h + parts[8].at);
    out->vox_pts = (const int32_t*)(h + parts[9].at);
    out->vox_av = (const float*)(h + parts[10].at);
    out->vox_cov = (const float*)(h + parts[11].at);
    return SCVOD_OK;
}

int host_scan(scvod_ctx* c, const float* h_xyzi, int32_t n, int do_pw, int filt, int do_vox, scvod_scan_result* out) {
    if (!c || !out || n < 0 || (n > 0 && !h_xyzi)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (n > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "%d points > capacity %lld", n, (long long)c->cap_pts);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc_side = ensure_side(c, kSideIn)) return rc_side;
    if (n) HIPCHK(c, hipMemcpyAsync(c->d_in, h_xyzi, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    int32_t off[2] = {0, n};
    int rc = run_batch(c, c->d_in, off, 1, c->stream, do_pw, filt, do_vox, 1);
    if (rc) return rc;
    rc = fetch_scan(c, 0, out);
    if (rc) return rc;
    if (!do_pw) out->n_patches = 0;
    return SCVOD_OK;
}

// ---- host-side pose algebra (pcl::getTransformation + Eigen::Affine3f inverse / product) ----
void get_transformation(const float p[6], float t[12]) {
    const float x = p[0], y = p[1], z = p[2], roll = p[3], pitch = p[4], yaw = p[5];
    const float A = std::cos(yaw), B = std::sin(yaw), C = std::cos(pitch), D = std::sin(pitch), E = std::cos(roll),
                F = std::sin(roll), DE = D * E, DF = D * F;
    t[0] = A * C;
    t[1] = A * DF - B * E;
    t[2] = B * F + A * DE;
    t[3] = x;
    t[4] = B * C;
    t[5] = A * E + B * DF;
    t[6] = B * DE - A * F;
    t[7] = y;
    t[8] = -D;
    t[9] = C * F;
    t[10] = C * E;
    t[11] = z;
}
inline float red3(float a, float b, float c) { return a + (b + c); }  // Eigen fixed-size redux order

// label filter + pcl::VoxelGrid over a batch of scans resident in HBM.  Two phases with one small host
// round trip each: the largest cell-index range picks the bucket shift of the voxel stage; the per-scan output counts
// become the output offsets.
int run_voxelgrid(scvod_ctx* c, const void* d_xyzi, const uint32_t* d_labels, const int32_t* h_off, int32_t n_scans,
                  const float leaf[3], float max_intensity, void* d_out, int64_t out_cap, int32_t* h_out_off, hipStream_t st) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_scans <= 0 || !h_off || !d_xyzi || !leaf || !d_out || !h_out_off) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    unmerge_view(c);
    if (!(leaf[0] > 0.f) || !(leaf[1] > 0.f) || !(leaf[2] > 0.f)) return fail(c, SCVOD_ERR_INVALID, "leaf size must be positive");
    if (n_scans > c->cap_scans) return fail(c, SCVOD_ERR_CAPACITY, "n_scans %d > capacity %d", n_scans, c->cap_scans);
    if (h_off[0] != 0) return fail(c, SCVOD_ERR_INVALID, "scan_offsets[0] must be 0");
    const int64_t total = h_off[n_scans];
    if (total > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "%lld points > capacity %lld", (long long)total, (long long)c->cap_pts);
    int32_t mx = 0;
    for (int s = 0; s < n_scans; ++s) {
        const int32_t n = h_off[s + 1] - h_off[s];
        if (n < 0) return fail(c, SCVOD_ERR_INVALID, "scan_offsets not monotone");
        if (n > mx) mx = n;
    }
    if (mx > SCVOD_MAX_SCAN_POINTS)
        return fail(c, SCVOD_ERR_CAPACITY, "scan of %d points > SCVOD_MAX_SCAN_POINTS (%d)", mx, SCVOD_MAX_SCAN_POINTS);
    HIPCHK(c, hipSetDevice(c->device));
    if (!st) st = c->stream;
    c->last_stream = st;
    join_lastname(c, st);
    c->h_scan_off.assign(h_off, h_off + n_scans + 1);
    HIPCHK(c, hipMemcpyAsync(c->d_scan_off, c->h_scan_off.data(), sizeof(int32_t) * (n_scans + 1), hipMemcpyHostToDevice, st));
    c->A.pts = (const float4*)d_xyzi;
    c->A.scan_off = c->d_scan_off;
    c->A.n_scans = n_scans;
    c->A.max_scan_pts = mx;
    c->A.total_pts = total;
    c->tim_used = 0;
    c->batch_valid = c->counts_valid = c->voxels_valid = c->clusters_valid = c->types_valid = c->track_valid = c->tables_valid = false;  // the arena is reused
    h_out_off[0] = 0;
    if (mx == 0) {
        for (int s = 0; s < n_scans; ++s) h_out_off[s + 1] = 0;
        return SCVOD_OK;
    }
    if (int rc_side = ensure_side(c, kSideApri)) return rc_side;  // (the centroids of a VoxelGrid run live in the PointAPRI array)
    VgJob J;
    J.labels = d_labels;
    J.max_intensity = max_intensity;
    for (int a = 0; a < 3; ++a) J.inv_leaf[a] = 1.0f / leaf[a];
    J.out = (float4*)d_out;
    // everything on the stream, one synchronisation at the end: bounding boxes + cell keys, the population-balanced
    // bucket table, the voxel stage in its centroid mode, output offsets, compaction into the caller's buffer
    Arena Av = c->A;
    Av.vb_lut = c->d_vb_lut;
    Av.vb_lut_shift = c->A.vg_range + 1;  // second word of the two-int scratch
    Av.vg_labels = d_labels;
    Av.vg_max_intensity = max_intensity;
    Av.vx_k32 = 0;  // cell indices are not bucket-relative: 64-bit sort keys
    DevParams D = c->dev;
    D.key_off = 0;
    D.vb_shift = 0;
    D.n_buckets = kMaxBuckets;
    launch_voxelgrid_keys(Av, J, st);
    launch_voxelgrid_lut(Av, st);
    launch_process(D, Av, st, 3, 0, 1, nullptr, nullptr);
    launch_voxelgrid_gather(D, Av, J, (long long)out_cap, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out_off, c->A.vg_outoff, sizeof(int32_t) * (n_scans + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (h_out_off[n_scans] > out_cap)
        return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%lld < %d points)", (long long)out_cap, h_out_off[n_scans]);
    return SCVOD_OK;
}

// Re-upload a small host table only when its contents changed since the last call (steady-state sequence loops pass the
// same tables every step and upload nothing).
// A changed table travels through one of eight pinned staging slots; a slot is reused only after the copy that read it
// has completed (its event), so a chunked sequence (scvod_sequence_ingest: new transforms every chunk) never drains the stream.
int staged_upload(scvod_ctx* c, const void* src, size_t bytes, void* dst, hipStream_t st) {
    UploadSlot& u = c->up_ring[c->up_next_slot];
    c->up_next_slot = (c->up_next_slot + 1) % 8;
    if (!u.ev) HIPCHK(c, hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
    if (u.used) HIPCHK(c, hipEventSynchronize(u.ev));
    if (bytes > u.cap) {
        if (u.pinned) hipHostFree(u.pinned);
        u.pinned = nullptr;
        u.cap = 0;
        HIPCHK(c, hipHostMalloc(&u.pinned, bytes + bytes / 2 + 64, hipHostMallocDefault));
        u.cap = bytes + bytes / 2 + 64;
    }
    memcpy(u.pinned, src, bytes);
    HIPCHK(c, hipMemcpyAsync(dst, u.pinned, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(u.ev, st));
    u.used = true;
    return SCVOD_OK;
}
template <typename T>
int upload_if_changed(scvod_ctx* c, std::vector<T>& held, const T* src, size_t n, void* dst, hipStream_t st) {
    if (held.size() == n && (n == 0 || memcmp(held.data(), src, n * sizeof(T)) == 0)) return SCVOD_OK;
    held.assign(src, src + n);
    return n ? staged_upload(c, held.data(), n * sizeof(T), dst, st) : SCVOD_OK;
}

// ---- sequential tracking chain: plan (chains of the successor table cut into segments) and workspace ----
size_t chain_layout(ChainWs& g, int max_scan_pts, int64_t pool_points) {
    const size_t nv = (size_t)(max_scan_pts > 0 ? max_scan_pts : 1);
    // appended clouds a state can hold: given, or 8 scans' worth (tracking CONSECUTIVE scans of a 10 Hz sequence keeps an object
    // in range for tens of frames and its cloud grows with every one of them -- the reference's own quadratic behaviour)
    size_t cap_pool = pool_points > 0 ? (size_t)pool_points : nv * 8;
    if (cap_pool < 65536) cap_pool = 65536;
    const size_t cap_ent = nv / 4 + 1024;
    g.cap_pool = (int32_t)cap_pool;
    g.cap_ent = (int32_t)cap_ent;
    g.cap_nv = (int32_t)nv;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off = align_up(off, 256);
        const size_t o = off;
        off += bytes;
        return o;
    };
    g.off_hdr = take(16 * 4);
    for (int i = 0; i < 3; ++i) {
        g.off_ent[i] = take(2 * cap_ent * sizeof(int4));
        g.off_parts[i] = take(cap_ent * 4);
        g.off_pool[i] = take(cap_pool * sizeof(float4));
    }
    g.off_chit = take(cap_pool * 4);
    g.off_evr = take(cap_ent * sizeof(int2));
    g.off_suniq = take((cap_pool + nv) * 4);
    g.off_spairs = take((cap_pool + nv) * sizeof(int2));
    g.off_vlab = take(nv * 8);
    g.off_lcnt = take((nv + cap_ent) * 8);
    g.off_lfwd = take((nv + cap_ent) * 8);
    g.off_newent = take(cap_ent * 4);
    g.off_cmeta = take(cap_ent * sizeof(int4));
    g.off_cparts = take(cap_ent * 4);
    g.off_links = take(cap_ent * sizeof(int4));
    g.off_dsz = take(2 * cap_ent * 4);
    g.off_eidx = take(2 * cap_ent * 4);
    g.off_rp = take(nv * sizeof(int2));
    g.stride = align_up(off, 4096);
    return g.stride;
}

// Chains = maximal runs scan -> successor -> ... inside the batch; every chain is cut into segments of `seg` steps, each
// walked by one workgroup that warms up `warm` steps earlier (scvod_chain.hip).  Returns the number of walkers, or a
// negative status when a scan is the successor of two scans (no sequence looks like that).
int plan_chains(scvod_ctx* c, const std::vector<int32_t>& next, std::vector<int32_t>& scans, std::vector<int32_t>& fw,
                std::vector<int32_t>& walkers) {
    const int B = (int)next.size();
    std::vector<int32_t> pred(B, -1);
    for (int s = 0; s < B; ++s)
        if (next[s] >= 0) {
            if (pred[next[s]] != -1) return fail(c, SCVOD_ERR_INVALID, "scan %d is the successor of scans %d and %d", next[s], pred[next[s]], s);
            if (next[s] == s) return fail(c, SCVOD_ERR_INVALID, "scan %d is its own successor", s);
            pred[next[s]] = s;
        }
    scans.clear();
    fw.assign(1, 0);
    walkers.clear();
    std::vector<char> seen(B, 0);
    // the chains: frames in order
    std::vector<int> chain_first, chain_len;
    for (int h = 0; h < B; ++h) {
        if (pred[h] != -1 || next[h] < 0) continue;  // not a head, or a head without a successor in the batch
        chain_first.push_back((int)scans.size());
        int n = 0;
        for (int s = h; s >= 0 && !seen[s]; s = next[s] >= 0 ? next[s] : -1) {
            seen[s] = 1;
            scans.push_back(s);
            ++n;
        }
        chain_len.push_back(n);
    }
    // segment length: given, or the SHORTEST whose segments still fit the device one per CU (a walker fills a CU; every walker
    // pays the warm-up, so more segments than CUs would run in two rounds) -- 11 steps = 255 walkers for seq 05 with skip_ 5
    int seg = c->chain_seg;
    if (seg <= 0) {
        const int n_cu = c->n_cu;
        int longest = 0;
        for (int n : chain_len) longest = n - 1 > longest ? n - 1 : longest;
        for (seg = 4; seg < longest; ++seg) {  // (more chains than CUs: one segment per chain)
            long long nseg = 0;
            for (int n : chain_len) nseg += (n - 1 + seg - 1) / seg;
            if (nseg <= n_cu) break;
        }
    }
    c->chain_seg_used = seg;
    if (c->chain_fb_pending && hipEventQuery(c->chain_fb_ev) == hipSuccess) {  // how the last batch of this stream fared
        c->chain_fb_pending = false;
        const int rewalked = c->h_chain_fb[1], limit = c->chain_fb_segments / 64 > 2 ? c->chain_fb_segments / 64 : 2;
        if (rewalked > limit && c->chain_warm_auto < 16) c->chain_warm_auto += 2;
    }
    const int warm = c->chain_warm >= 0 ? c->chain_warm : c->chain_warm_auto;
    c->chain_warm_used = warm;
    // the times the walkers of this stream's last batch measured per step (same plan of frames): a kernel lasts as long as its slowest
    // walker, and what a step costs follows the stretch of the sequence (objects tracked for tens of frames carry large clouds), not
    // anything the planner could read off the scans -- so the segments of the NEXT batch are cut to equal measured time (warm-up included)
    if (c->step_fb_pending && hipEventQuery(c->step_fb_ev) == hipSuccess) {
        c->step_fb_pending = false;
        c->step_ticks.assign(c->h_step_ticks, c->h_step_ticks + c->step_fb_scans.size());
        c->step_ticks_scans = c->step_fb_scans;
    }
    std::vector<std::vector<int>> cuts;  // per chain: segment starts (own steps), when cut by time
    // (planned ONCE per plan of frames, halo and warm-up -- from the first times that arrive for it -- and kept: the host pays for the
    //  search once, the walker table is uploaded once, and a stream's batches keep one segmentation)
    if (c->chain_seg <= 0 && c->chain_balance && !c->cuts_cache.empty() && c->cuts_scans == scans && c->cuts_chain_first == chain_first &&
        c->cuts_chain_len == chain_len && c->cuts_warm == warm && c->cuts_halo == c->halo) {
        cuts = c->cuts_cache;
    } else if (c->chain_seg <= 0 && c->chain_balance && !c->step_ticks.empty() && c->step_ticks_scans == scans) {
        std::vector<double> cost(scans.size(), 0.0);
        double sum = 0;
        long long cnt = 0;
        for (size_t i = 0; i < scans.size(); ++i)
            if (c->step_ticks[i] > 0) {
                sum += c->step_ticks[i];
                ++cnt;
            }
        const double mean = cnt ? sum / (double)cnt : 1.0;
        for (size_t i = 0; i < scans.size(); ++i) cost[i] = c->step_ticks[i] > 0 ? (double)c->step_ticks[i] : mean;
        std::vector<int> a0s(chain_len.size());
        double total = 0, biggest = 0;
        for (size_t ci = 0; ci < chain_len.size(); ++ci) {
            const int first = chain_first[ci], steps = chain_len[ci] - 1;
            int a0 = 0;
            while (a0 < steps && (size_t)scans[first + a0] < c->halo.size() && c->halo[scans[first + a0]]) ++a0;
            a0s[ci] = a0;
            for (int k = 0; k < steps; ++k) total += cost[first + k];
        }
        auto plan = [&](double tau, std::vector<std::vector<int>>* out) -> long long {
            long long nseg = 0;
            if (out) out->assign(chain_len.size(), std::vector<int>());
            for (size_t ci = 0; ci < chain_len.size(); ++ci) {
                const int first = chain_first[ci], steps = chain_len[ci] - 1, a0 = a0s[ci];
                int a = a0;
                while (a < steps) {
                    const int t0 = (a == a0 && a0 > 0) ? 0 : (a - warm > 0 ? a - warm : 0);
                    double t = 0;
                    for (int k = t0; k < a; ++k) t += cost[first + k];
                    int b = a;
                    do {
                        t += cost[first + b];
                        ++b;
                    } while (b < steps && t + cost[first + b] <= tau);
                    if (out) (*out)[ci].push_back(a);
                    ++nseg;
                    a = b;
                }
            }
            return nseg;
        };
        double lo_t = 0, hi_t = total + 1.0;  // smallest tau whose plan fits the device one walker per CU
        if (plan(hi_t, nullptr) <= c->n_cu) {
            for (int it = 0; it < 40; ++it) {
                const double mid = 0.5 * (lo_t + hi_t);
                if (plan(mid, nullptr) <= c->n_cu)
                    hi_t = mid;
                else
                    lo_t = mid;
            }
            plan(hi_t, &cuts);
            c->cuts_cache = cuts;
            c->cuts_scans = scans;
            c->cuts_chain_first = chain_first;
            c->cuts_chain_len = chain_len;
            c->cuts_warm = warm;
            c->cuts_halo = c->halo;
        }
    }
    if (!cuts.empty()) {  // cuts that do not describe THIS plan (one list per chain, ascending starts inside the chain's steps): equal-length segments instead
        bool ok = cuts.size() == chain_len.size();
        for (size_t ci = 0; ok && ci < cuts.size(); ++ci) {
            int prev = -1;
            for (int a : cuts[ci]) {
                if (a <= prev || a >= chain_len[ci] - 1) ok = false;
                prev = a;
            }
        }
        if (!ok) {
            cuts.clear();
            c->cuts_cache.clear();
        }
    }
    int n_chains = 0;
    for (size_t ci = 0; ci < chain_len.size(); ++ci) {
        const int first = chain_first[ci], n = chain_len[ci];
        const int steps = n - 1;
        // frames of a halo (scvod_set_track_owned): the chain's own steps start at its first frame that is not one; the steps before
        // are only ever a warm-up (the whole halo for the first walker: its start state has no other source on this shard)
        int a0 = 0;
        while (a0 < steps && (size_t)scans[first + a0] < c->halo.size() && c->halo[scans[first + a0]]) ++a0;
        for (int a = a0; a < n; ++a)  // a halo flag behind a scan of the chain that is not halo would be ignored silently: refuse it
            if ((size_t)scans[first + a] < c->halo.size() && c->halo[scans[first + a]] && a > a0)
                return fail(c, SCVOD_ERR_INVALID, "scan %d is marked halo but follows scan %d of its chain, which is not: a chain's halo scans must be its first ones", scans[first + a], scans[first + a0]);
        if (!cuts.empty()) {
            const std::vector<int>& cs = cuts[ci];
            for (size_t k = 0; k < cs.size(); ++k) {
                const int a = cs[k], b = k + 1 < cs.size() ? cs[k + 1] : steps;
                const int t0 = (a == a0 && a0 > 0) ? 0 : (a - warm > 0 ? a - warm : 0);
                const int32_t w[8] = {first, n, a, b, t0, n_chains, (a == a0 && a0 > 0) ? 1 : 0, 0};
                walkers.insert(walkers.end(), w, w + 8);
            }
            fw.push_back((int32_t)(walkers.size() / 8));
            ++n_chains;
            continue;
        }
        for (int a = a0; a < steps; a += seg) {
            const int b = a + seg < steps ? a + seg : steps;
            const int t0 = (a == a0 && a0 > 0) ? 0 : (a - warm > 0 ? a - warm : 0);
            const int32_t w[8] = {first, n, a, b, t0, n_chains, (a == a0 && a0 > 0) ? 1 : 0, 0};
            walkers.insert(walkers.end(), w, w + 8);
        }
        fw.push_back((int32_t)(walkers.size() / 8));
        ++n_chains;
    }
    // (a cycle has no head: its scans keep their first-order result; rejected here to be explicit)
    for (int s = 0; s < B; ++s)
        if (next[s] >= 0 && !seen[s]) return fail(c, SCVOD_ERR_INVALID, "the successor table holds a cycle through scan %d", s);
    return (int)(walkers.size() / 8);
}

}  // namespace

// internal bridge for scvod_map.hip (not part of the public header)
extern "C" int scvod__ctx_types_valid(scvod_ctx* c) { return (c->clusters_valid && c->types_valid) ? 1 : 0; }
extern "C" int scvod__ctx_view(scvod_ctx* c, Arena* arena, int* device, int* track_valid, int* batch_valid, int* n_scans,
                               int* max_scan_pts, int* batch_mode, int* num_min_pts) {
    *batch_mode = c->batch_mode;
    *num_min_pts = c->pw.num_min_pts;
    *arena = c->A;
    *device = c->device;
    *track_valid = c->track_valid ? 1 : 0;
    *batch_valid = (c->batch_valid && c->batch_mode != 3) ? 1 : 0;
    *n_scans = c->A.n_scans;
    *max_scan_pts = c->A.max_scan_pts;
    return 0;
}
// the stream a stream-ordered batch call runs on: the caller's, or (NULL) the stream of the ctx's last batch call
// the three index lists of the batch, written before anything queued on `stream` behind this call reads them (k_map_mark_lists)
extern "C" int scvod__ctx_ensure_lists(scvod_ctx* c, void* stream) { return ensure_lists(c, (hipStream_t)stream); }
extern "C" void* scvod__ctx_stream(scvod_ctx* c, void* stream) { return stream ? stream : (void*)(c->last_stream ? c->last_stream : c->stream); }
// scvod_register.hip: where its state hangs on the ctx, the ctx's device and own stream, and its error text
extern "C" void** scvod__ctx_register_slot(scvod_ctx* c, int* device, void** own_stream) {
    *device = c->device;
    *own_stream = (void*)c->stream;
    return &c->reg_state;
}
// scvod_normals.hip: the same for its state
extern "C" void** scvod__ctx_normals_slot(scvod_ctx* c, int* device, void** own_stream) {
    *device = c->device;
    *own_stream = (void*)c->stream;
    return &c->nrm_state;
}
extern "C" int scvod__ctx_fail(scvod_ctx* c, int code, const char* msg) { return fail(c, code, "%s", msg); }

extern "C" {

void scvod_params_default(scvod_params* p) {
    memset(p, 0, sizeof(*p));
    p->sensor_height = 2.0f;
    p->min_dis = 0.0f;
    p->max_dis = 50.0f;
    p->min_angle = 0.0f;
    p->max_angle = 360.0f;
    p->min_azimuth = -30.0f;
    p->max_azimuth = 60.0f;
    p->range_res = 0.2f;
    p->sector_res = 1.2f;
    p->azimuth_res = 2.0f;
    p->occupancy = 0.6f;
    p->max_z = 1.0f;       // utility.h:294
    p->min_z = -1.0f;      // utility.h:295
    p->car_square = 2.0f;  // utility.h:298
    p->toBeClass = 1;      // utility.h:306
}

void scvod_pw_params_default(scvod_pw_params* p) {
    memset(p, 0, sizeof(*p));
    p->num_iter = 3;
    p->num_lpr = 20;
    p->num_min_pts = 10;
    p->num_rings_of_interest = 4;
    const int sec[4] = {16, 32, 54, 32}, rng[4] = {2, 4, 4, 4};
    const double el[4] = {-1.2, -0.9984, -0.851, -0.605}, fl[4] = {0.0, 0.000125, 0.000185, 0.000185};
    for (int i = 0; i < 4; ++i) {
        p->num_sectors_each_zone[i] = sec[i];
        p->num_rings_each_zone[i] = rng[i];
        p->elevation_thr[i] = el[i];
        p->flatness_thr[i] = fl[i];
    }
    p->th_seeds = 0.3;
    p->th_dist = 0.1;
    p->max_range = 80.0;
    p->min_range = 2.7;
    p->uprightness_thr = 0.707;
    p->adaptive_seed_selection_margin = -1.1;
}

void scvod_grid_dims(const scvod_params* p, int32_t* range_num, int32_t* sector_num, int32_t* azimuth_num,
                     int32_t* bin_num) {
    // src/ssc.cpp:36-39: float arithmetic, std::ceil(float)
    const int r = (int)std::ceil((p->max_dis - p->min_dis) / p->range_res);
    const int s = (int)std::ceil((p->max_angle - p->min_angle) / p->sector_res);
    const int a = (int)std::ceil((p->max_azimuth - p->min_azimuth) / p->azimuth_res);
    if (range_num) *range_num = r;
    if (sector_num) *sector_num = s;
    if (azimuth_num) *azimuth_num = a;
    if (bin_num) *bin_num = r * s * a;
}

int scvod_create(const scvod_params* params, const scvod_pw_params* pw, int device, int64_t max_points_total,
                 int32_t max_scans, scvod_ctx** out) {
    if (!params || !out || max_points_total <= 0 || max_scans <= 0) return SCVOD_ERR_INVALID;
    *out = nullptr;
    if (max_points_total > 2147483583ll) return SCVOD_ERR_CAPACITY;  // scan offsets and point indices are int32
    scvod_ctx* c = new scvod_ctx();
    c->device = device;
    c->params = *params;
    if (pw)
        c->pw = *pw;
    else
        scvod_pw_params_default(&c->pw);
    int np = 0;
    for (int k = 0; k < 4; ++k) {
        if (c->pw.num_rings_each_zone[k] <= 0 || c->pw.num_sectors_each_zone[k] <= 0) {
            delete c;
            return SCVOD_ERR_INVALID;
        }
        np += c->pw.num_rings_each_zone[k] * c->pw.num_sectors_each_zone[k];
    }
    // the elevation / flatness gates are indexed ring + 2 * zone for the patches of the first num_rings_of_interest
    // concentric rings (patchwork.h:351-353) and hold four entries (patchwork.h:50-51): a layout that would index past
    // them reads out of bounds in the reference; refused here
    {
        int conc = 0;
        for (int k = 0; k < 4; ++k)
            for (int r = 0; r < c->pw.num_rings_each_zone[k]; ++r, ++conc)
                if (conc < c->pw.num_rings_of_interest && r + 2 * k > 3) {
                    delete c;
                    return SCVOD_ERR_INVALID;
                }
    }
    // th_seeds < 0 or a near-zero th_dist could leave a plane iteration without points: the reference then fits with the
    // stale moments of the previous patch (PCL leaves cov / mean untouched for an empty cloud) -- not modelled, refused
    if (np > kMaxPatches || !(params->range_res > 0) || !(params->sector_res > 0) || !(params->azimuth_res > 0) ||
        !(c->pw.th_seeds >= 0.0) || !(c->pw.th_dist >= 0.01) || c->pw.num_iter < 1 || c->pw.num_lpr < 1) {
        delete c;
        return SCVOD_ERR_INVALID;
    }
    int ndev = 0;  // (argument errors are reported before the device is looked for)
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        delete c;
        return SCVOD_ERR_NO_DEVICE;
    }
    c->cap_pts = max_points_total;
    c->cap_scans = max_scans;
    build_dev_params(c);
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return SCVOD_ERR_NO_DEVICE;
    }
    size_t total = 0;
    carve(c, nullptr, &total);
    if (hipMalloc(&c->arena_base, total) != hipSuccess) {
        delete c;
        return SCVOD_ERR_HIP;
    }
    c->arena_bytes = total;
    carve(c, (unsigned char*)c->arena_base, &total);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        if (const char* e = getenv("SCVOD_CHAIN_BALANCE")) c->chain_balance = atoi(e);  // (development: 0 = equal-length segments, as rounds 3-4)
    }
    if (hipStreamCreate(&c->stream) != hipSuccess) {
        hipFree(c->arena_base);
        delete c;
        return SCVOD_ERR_HIP;
    }
    *out = c;
    return SCVOD_OK;
}

void scvod_destroy(scvod_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (auto& t : c->tim) {
        hipEventDestroy(t.e0);
        hipEventDestroy(t.e1);
    }
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->ln_stream) hipStreamDestroy(c->ln_stream);
    if (c->h_chain_fb) hipHostFree(c->h_chain_fb);
    if (c->h_step_ticks) hipHostFree(c->h_step_ticks);
    if (c->h_ext_state_pin) hipHostFree(c->h_ext_state_pin);
    if (c->step_fb_ev) hipEventDestroy(c->step_fb_ev);
    if (c->chain_fb_ev) hipEventDestroy(c->chain_fb_ev);
    if (c->ln_stream2) hipStreamDestroy(c->ln_stream2);
    if (c->ln_stream3) hipStreamDestroy(c->ln_stream3);
    if (c->ln_join3) hipEventDestroy(c->ln_join3);
    if (c->ln_fork2) hipEventDestroy(c->ln_fork2);
    if (c->ln_join2) hipEventDestroy(c->ln_join2);
    if (c->ln_fork) hipEventDestroy(c->ln_fork);
    if (c->ln_done) hipEventDestroy(c->ln_done);
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    for (int k = 0; k < 2; ++k) {
        if (c->ingest_buf[k]) hipFree(c->ingest_buf[k]);
        if (c->ingest_copied[k]) hipEventDestroy(c->ingest_copied[k]);
        if (c->ingest_done[k]) hipEventDestroy(c->ingest_done[k]);
    }
    if (c->ingest_off) hipHostFree(c->ingest_off);
    for (UploadSlot& u : c->up_ring) {
        if (u.pinned) hipHostFree(u.pinned);
        if (u.ev) hipEventDestroy(u.ev);
    }
    if (c->arena_base) hipFree(c->arena_base);
    if (c->d_in) hipFree(c->d_in);
    if (c->t_pts) hipFree(c->t_pts);
    if (c->d_labels) hipFree(c->d_labels);
    if (c->d_apri) hipFree(c->d_apri);
    if (c->im_buf) hipFree(c->im_buf);
    if (c->rg_buf) hipFree(c->rg_buf);
    if (c->rg_sort_tmp) hipFree(c->rg_sort_tmp);
    if (c->rg_out) hipFree(c->rg_out);
    if (c->rg_ev) hipEventDestroy(c->rg_ev);
    if (c->cal_buf) hipFree(c->cal_buf);
    if (c->cal_fetch) hipFree(c->cal_fetch);
    if (c->chain_ws) hipFree(c->chain_ws);
    if (c->exp_labels) hipFree(c->exp_labels);
    if (c->exp_scan_cnt) hipFree(c->exp_scan_cnt);
    if (c->exp_pose) hipFree(c->exp_pose);
    if (c->exp_stats) hipFree(c->exp_stats);
    if (c->exp_tiles) hipFree(c->exp_tiles);
    if (c->obj_scan_cnt) hipFree(c->obj_scan_cnt);
    if (c->obj_stats) hipFree(c->obj_stats);
    if (c->obj_tiles) hipFree(c->obj_tiles);
    if (c->obj_keys) hipFree(c->obj_keys);
    if (c->obj_words) hipFree(c->obj_words);
    if (c->obj_sort_tmp) hipFree(c->obj_sort_tmp);
    if (c->shape_stats) hipFree(c->shape_stats);
    if (c->ev.buf) hipFree(c->ev.buf);
    if (c->ev_counters) hipFree(c->ev_counters);
    if (c->cs.buf) hipFree(c->cs.buf);
    if (c->cs_counters) hipFree(c->cs_counters);
    if (c->in.buf) hipFree(c->in.buf);
    if (c->in_counters) hipFree(c->in_counters);
    if (c->ot.buf) hipFree(c->ot.buf);
    if (c->ot_counters) hipFree(c->ot_counters);
    if (c->esf.buf) hipFree(c->esf.buf);
    if (c->esf_counters) hipFree(c->esf_counters);
    if (c->esf_ev) hipEventDestroy(c->esf_ev);
    scvod__register_free(c->reg_state);
    scvod__normals_free(c->nrm_state);
    if (c->ov.buf) hipFree(c->ov.buf);
    if (c->ov_counters) hipFree(c->ov_counters);
    if (c->trk.buf) hipFree(c->trk.buf);
    if (c->trk_counters) hipFree(c->trk_counters);
    if (c->tv.buf) hipFree(c->tv.buf);
    if (c->tv_counters) hipFree(c->tv_counters);
    if (c->stk.buf) hipFree(c->stk.buf);
    if (c->vis.buf) hipFree(c->vis.buf);
    if (c->vis_counters) hipFree(c->vis_counters);
    if (c->cv.buf) hipFree(c->cv.buf);
    if (c->cv_counters) hipFree(c->cv_counters);
    if (c->sp.buf) hipFree(c->sp.buf);
    if (c->sp_stats) hipFree(c->sp_stats);
    if (c->stage) hipHostFree(c->stage);
    for (const Scratch& s : c->nn)
        if (s.buf) hipFree(s.buf);
    delete c;
}

const char* scvod_last_error(const scvod_ctx* c) { return c ? c->err.c_str() : "null ctx"; }
int64_t scvod_arena_bytes(const scvod_ctx* c) { return c ? (int64_t)(c->arena_bytes + c->side_bytes) : 0; }

int scvod_process_scan(scvod_ctx* c, const float* h_xyzi, int32_t n, scvod_scan_result* out) {
    return host_scan(c, h_xyzi, n, 1, 1, 1, out);
}
int scvod_patchwork(scvod_ctx* c, const float* h_xyzi, int32_t n, scvod_scan_result* out) {
    int rc = host_scan(c, h_xyzi, n, 1, 1, 0, out);
    if (rc == SCVOD_OK) {
        out->n_apri = out->n_rejected = out->n_voxels = 0;
    }
    return rc;
}
int scvod_bin_scan(scvod_ctx* c, const float* h_xyzi, int32_t n, int32_t apply_filter, int32_t with_voxels,
                   scvod_scan_result* out) {
    return host_scan(c, h_xyzi, n, 0, apply_filter ? 1 : 0, with_voxels ? 1 : 0, out);
}

int scvod_voxelize(scvod_ctx* c, const scvod_apri* h_apri, int32_t n, scvod_scan_result* out) {
    if (!c || !out || n < 0 || (n > 0 && !h_apri)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (n > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "%d points > capacity %lld", n, (long long)c->cap_pts);
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t counts[8] = {n, 0, 0, 0, n, 0, 0, 0};
    if (int rc_side = ensure_side(c, kSideApri)) return rc_side;
    if (n) HIPCHK(c, hipMemcpyAsync(c->A.apri, h_apri, sizeof(scvod_apri) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->A.counts, counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int32_t off[2] = {0, n};
    int rc = run_batch(c, nullptr, off, 1, c->stream, 2, 0, 1, 1);
    if (rc) return rc;
    rc = fetch_scan(c, 0, out);
    if (rc) return rc;
    out->n_patches = 0;
    return SCVOD_OK;
}

void scvod_pose_delta(const float pose_pre[6], const float pose_next[6], float T_out[12]) {
    float tn[12], tp[12];
    get_transformation(pose_next, tn);
    get_transformation(pose_pre, tp);
    // Eigen::Affine3f::inverse(): cofactor inverse of the linear part, then -R^-1 * t
    auto M = [&](int i, int j) { return tn[4 * i + j]; };
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return M(i1, j1) * M(i2, j2) - M(i1, j2) * M(i2, j1);
    };
    const float c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
    const float det = red3(c0 * M(0, 0), c1 * M(1, 0), c2 * M(2, 0));
    const float invdet = 1.f / det;
    float R[3][3];
    R[0][0] = c0 * invdet;
    R[0][1] = c1 * invdet;
    R[0][2] = c2 * invdet;
    R[1][0] = cof(0, 1) * invdet;
    R[1][1] = cof(1, 1) * invdet;
    R[1][2] = cof(2, 1) * invdet;
    R[2][0] = cof(0, 2) * invdet;
    R[2][1] = cof(1, 2) * invdet;
    R[2][2] = cof(2, 2) * invdet;
    float ti[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) ti[4 * i + j] = R[i][j];
        ti[4 * i + 3] = red3((-R[i][0]) * tn[3], (-R[i][1]) * tn[7], (-R[i][2]) * tn[11]);
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            T_out[4 * i + j] = red3(ti[4 * i] * tp[j], ti[4 * i + 1] * tp[4 + j], ti[4 * i + 2] * tp[8 + j]);
        T_out[4 * i + 3] = red3(ti[4 * i] * tp[3], ti[4 * i + 1] * tp[7], ti[4 * i + 2] * tp[11]) + ti[4 * i + 3];
    }
}

int scvod_track_probe(scvod_ctx* c, const float* h_xyzi, const int32_t* h_offsets, int32_t n_clusters, const float T[12],
                      const int32_t* h_next_keys, const int32_t* h_next_labels, int32_t n_next_vox, int32_t* h_hit_slot,
                      int32_t* h_uniq_slots, int32_t* h_uniq_begin) {
    if (!c || n_clusters < 0 || !h_offsets || !T || n_next_vox < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (h_offsets[0] != 0) return fail(c, SCVOD_ERR_INVALID, "cluster offsets must start at 0");
    for (int k = 0; k < n_clusters; ++k)
        if (h_offsets[k + 1] < h_offsets[k]) return fail(c, SCVOD_ERR_INVALID, "cluster offsets not monotone");
    const int32_t n_pts = h_offsets[n_clusters];
    if ((n_pts > 0 && !h_xyzi) || (n_next_vox > 0 && !h_next_keys)) return fail(c, SCVOD_ERR_INVALID, "null input array");
    if (n_pts > c->cap_pts || n_clusters > c->cap_pts || n_next_vox > c->cap_pts)
        return fail(c, SCVOD_ERR_CAPACITY, "track probe larger than the ctx capacity");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->last_stream = st;
    join_lastname(c, st);
    c->tim_used = 0;
    // the one-shot probe writes t_T and scratch that scvod_batch_track's results alias: forget the cached upload of T and
    // the batch's tracking result (a following scvod_batch_track uploads and decides again)
    c->up_T.clear();
    c->track_valid = false;
    if (int rc_side = ensure_side(c, kSideTpts)) return rc_side;
    float4* d_pts = c->t_pts;
    if (n_pts) HIPCHK(c, hipMemcpyAsync(d_pts, h_xyzi, sizeof(float) * 4 * (size_t)n_pts, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->t_begin, h_offsets, sizeof(int32_t) * (n_clusters + 1), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->t_T, T, sizeof(float) * 12, hipMemcpyHostToDevice, st));
    if (n_next_vox) {
        HIPCHK(c, hipMemcpyAsync(c->A.tmp_vox_key, h_next_keys, sizeof(int32_t) * n_next_vox, hipMemcpyHostToDevice, st));
        if (h_next_labels)
            HIPCHK(c, hipMemcpyAsync(c->A.tmp_vox_begin, h_next_labels, sizeof(int32_t) * n_next_vox, hipMemcpyHostToDevice, st));
    }
    TrackJob J;
    memset(&J, 0, sizeof(J));
    J.pts = d_pts;
    J.pt_cluster_begin = c->t_begin;
    J.n_clusters = n_clusters;
    J.n_pts = n_pts;
    J.T = c->t_T;
    J.next_keys = c->A.tmp_vox_key;
    J.next_labels = h_next_labels ? c->A.tmp_vox_begin : nullptr;
    J.n_next_vox = n_next_vox;
    J.hit_slot = c->t_hit;
    J.work = c->t_work;
    J.uniq_slots = c->t_uniq;
    J.uniq_count = c->t_count;
    launch_track(c->dev, c->A, J, 0, st, timer_hook, c);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    if (n_pts && h_hit_slot) HIPCHK(c, hipMemcpy(h_hit_slot, c->t_hit, sizeof(int32_t) * n_pts, hipMemcpyDeviceToHost));
    std::vector<int32_t> cnt(n_clusters > 0 ? n_clusters : 1), uq(n_pts > 0 ? n_pts : 1);
    if (n_clusters) HIPCHK(c, hipMemcpy(cnt.data(), c->t_count, sizeof(int32_t) * n_clusters, hipMemcpyDeviceToHost));
    if (n_pts) HIPCHK(c, hipMemcpy(uq.data(), c->t_uniq, sizeof(int32_t) * n_pts, hipMemcpyDeviceToHost));
    int32_t o = 0;
    for (int k = 0; k < n_clusters; ++k) {
        if (h_uniq_begin) h_uniq_begin[k] = o;
        for (int j = 0; j < cnt[k]; ++j) {
            if (h_uniq_slots) h_uniq_slots[o] = uq[h_offsets[k] + j];
            ++o;
        }
    }
    if (h_uniq_begin) h_uniq_begin[n_clusters] = o;
    return SCVOD_OK;
}

int scvod_batch_process(scvod_ctx* c, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, void* stream,
                        int32_t sync) {
    return run_batch(c, d_xyzi, h_scan_offsets, n_scans, (hipStream_t)stream, 1, 1, 1, sync, false, true);
}

int scvod_batch_counts(scvod_ctx* c, int32_t* h_out) {
    if (!c || !h_out) return SCVOD_ERR_INVALID;
    int rc = ensure_counts(c);
    if (rc) return rc;
    memcpy(h_out, c->h_counts.data(), sizeof(int32_t) * c->h_counts.size());
    return SCVOD_OK;
}

int scvod_batch_fetch(scvod_ctx* c, int32_t s, scvod_scan_result* out) {
    if (!c || !out) return SCVOD_ERR_INVALID;
    return fetch_scan(c, s, out);
}

int scvod_batch_cluster(scvod_ctx* c, void* stream, int32_t sync) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->batch_valid || !c->voxels_valid)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_cluster needs a processed batch with voxel descriptors");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    c->last_stream = st;
    c->tim_used = 0;
    if (c->dev.bin.range_num > 2040 || c->dev.bin.sector_num > 2040 || c->dev.bin.azimuth_num > 1016)
        return fail(c, SCVOD_ERR_INVALID, "grid of %d x %d x %d bins is finer than the clustering's packed index triples hold (2040 x 2040 x 1016)",
                    c->dev.bin.range_num, c->dev.bin.sector_num, c->dev.bin.azimuth_num);
    join_lastname(c, st);
    // a second clustering of the same batch (other mode, scvod_set_cluster_exact, cluster - track - cluster): the marks the first one
    // and its tracking left per input point would otherwise survive on points that are no car members any more
    if (c->clustered_this_batch && c->A.total_pts > 0) HIPCHK(c, hipMemsetAsync(c->A.pt_mapcls, 0, (size_t)c->A.total_pts, st));
    c->clustered_this_batch = true;
    unmerge_view(c);
    if (!c->pt_cluster_own) c->pt_cluster_own = c->A.pt_cluster;
    if (c->im_iterations > 0) {
        const size_t lds = merge_lds_bytes(c->dev, c->A.max_scan_pts);
        if (lds > 160 * 1024 - 256)
            return fail(c, SCVOD_ERR_INVALID, "intensity merge: %zu bytes of LDS for a %d x %d row table and scans of %d points (160 KB per workgroup)",
                        lds, c->dev.bin.range_num, c->dev.bin.azimuth_num, c->A.max_scan_pts);
        int rc = ensure_merge(c);
        if (rc) return rc;
    }
    // the max_name pass takes its arena scratch from whichever of {seg, the three index lists} is not needed any more (ensure_lists)
    c->A.ln_scratch = c->lists_valid ? c->A.seg : (uint32_t*)c->A.ground_idx;
    launch_cluster(c->dev, c->A, c->batch_mode == 2 ? 1 : 0, st, timer_hook, c);
    if (c->im_iterations > 0) {  // (before the max_name passes: they read pt_cluster, left as it was, and the post-merge pt_type)
        if (int rc_desc = ensure_descriptors(c, st)) return rc_desc;  // (the merge compares vox_av / vox_cov)
        c->im.iterations = c->im_iterations;
        c->im.search_c = c->im_search_c;
        c->im.diff = c->im_diff;
        c->im.cov = c->im_cov;
        launch_merge(c->dev, c->A, c->im, c->batch_mode == 2 ? 1 : 0, st, timer_hook, c);
        c->merged = true;
    }
    // (the max_name passes below still read the pre-merge partition: they take c->A by value before the view switches)
    c->last_name_valid = false;
    // Frame::max_name of every scan (scvod_lastname.hip): launches of its own beside the tracking kernels.  (Run by the clustering
    // workgroup itself -- 1024 threads, one workgroup per CU -- the pass is a chain of dependent look-ups nobody hides: measured
    // in round 4, k_cc_scan 3.1 -> 7.6 ms; as separate passes with eight small workgroups per CU it costs 3 ms, partly hidden.)
    if (c->max_name_literal) {
        if (!c->ln_stream) {
            // (highest priority: the few workgroups of these passes -- one per scan that needs one, each a chain of dependent
            // look-ups -- are dispatched ahead of the tracking kernels' thousands and finish while those stream)
            int prio_low = 0, prio_high = 0;
            HIPCHK(c, hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
            if (getenv("SCVOD_LN_NO_PRIORITY")) prio_high = prio_low;
            HIPCHK(c, hipStreamCreateWithPriority(&c->ln_stream, hipStreamNonBlocking, prio_high));
            HIPCHK(c, hipEventCreateWithFlags(&c->ln_fork, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ln_done, hipEventDisableTiming));
            HIPCHK(c, hipStreamCreateWithPriority(&c->ln_stream2, hipStreamNonBlocking, prio_high));
            HIPCHK(c, hipEventCreateWithFlags(&c->ln_fork2, hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->ln_join2, hipEventDisableTiming));
            HIPCHK(c, hipStreamCreateWithPriority(&c->ln_stream3, hipStreamNonBlocking, prio_high));
            HIPCHK(c, hipEventCreateWithFlags(&c->ln_join3, hipEventDisableTiming));
        }
        if (c->timing) {  // attribution runs: one stream, one pair of events per pass
            launch_lastname(c->dev, c->A, st, nullptr, nullptr, nullptr, nullptr, nullptr, timer_hook, c);
            if (c->merged) launch_merge_lastname(c->A, c->im, st, timer_hook, c);
        } else {
            HIPCHK(c, hipEventRecord(c->ln_fork, st));
            HIPCHK(c, hipStreamWaitEvent(c->ln_stream, c->ln_fork, 0));
            launch_lastname(c->dev, c->A, c->ln_stream, c->ln_stream2, c->ln_stream3, c->ln_fork2, c->ln_join2, c->ln_join3, nullptr, c);
            if (c->merged) launch_merge_lastname(c->A, c->im, c->ln_stream, nullptr, c);
            HIPCHK(c, hipEventRecord(c->ln_done, c->ln_stream));
            c->ln_pending = true;
        }
        c->last_name_valid = true;
        if (sync) join_lastname(c, st);
    }
    if (c->merged) c->A.pt_cluster = c->im.pt_merged;
    HIPCHK(c, hipGetLastError());
    c->clusters_valid = true;
    ++c->cluster_serial;
    c->types_valid = false;  // scvod_batch_cluster_types publishes them
    c->track_valid = false;
    c->tables_valid = false;
    if (sync) HIPCHK(c, hipStreamSynchronize(st));
    return SCVOD_OK;
}

int scvod_batch_fetch_clusters(scvod_ctx* c, int32_t s, int32_t* h_pt_cluster, int32_t cap) {
    if (!c || !h_pt_cluster) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "no clusters computed for the last batch");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t n = c->h_counts[(size_t)s * 8 + 4];
    if (n > cap) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    if ((rc = merge_check(c))) return rc;
    if (n) HIPCHK(c, hipMemcpy(h_pt_cluster, c->A.pt_cluster + c->h_scan_off[s], sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return n;
}

int scvod_batch_cluster_types(scvod_ctx* c, void* stream, int32_t sync) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "scvod_batch_cluster_types needs scvod_batch_cluster first");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    hipStream_t prev = c->last_stream;
    c->last_stream = st;
    // (nothing is launched here: the max_name pass keeps running beside what follows)
    c->tim_used = 0;
    // the boxes and the type rules are evaluated by the clustering kernel itself (same workgroup, boxes in LDS): nothing to launch,
    // unless the region growing is on (scvod_k_rgrow.inc)
    c->rg_done = false;
    ++c->types_serial;
    if (c->rg_on) {
        if (int rc = merge_check(c)) return rc;
        int rc = ensure_rgrow(c, 1);
        if (rc) return rc;
        if (prev && prev != st) {  // the clustering ran on another stream
            HIPCHK(c, hipEventRecord(c->rg_ev, prev));
            HIPCHK(c, hipStreamWaitEvent(st, c->rg_ev, 0));
        }
        if ((rc = run_rgrow(c, st))) return rc;
        c->rg_done = true;
    }
    c->types_valid = true;
    c->track_valid = false;
    c->tables_valid = false;
    if (sync) HIPCHK(c, hipStreamSynchronize(st));
    return SCVOD_OK;
}

int scvod_batch_fetch_cluster_types(scvod_ctx* c, int32_t s, int32_t car_label, int32_t other_label, int32_t* h_type,
                                    int32_t cap) {
    if (!c || !h_type) return SCVOD_ERR_INVALID;
    if (!c->types_valid) return fail(c, SCVOD_ERR_STATE, "no cluster types computed for the last batch");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t n = c->h_counts[(size_t)s * 8 + 4];
    if (n > cap) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    if ((rc = merge_check(c))) return rc;
    std::vector<uint8_t> t(n ? n : 1);
    if (n) HIPCHK(c, hipMemcpy(t.data(), c->A.pt_type + c->h_scan_off[s], (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) h_type[i] = t[i] == 0 ? -1 : (t[i] == 2 ? car_label : other_label);
    return n;
}

int scvod_batch_fetch_cluster_classes(scvod_ctx* c, int32_t s, int32_t car_label, int32_t building_label, int32_t tree_label,
                                      int32_t* h_type, int32_t cap) {
    if (!c || !h_type) return SCVOD_ERR_INVALID;
    if (!c->types_valid) return fail(c, SCVOD_ERR_STATE, "no cluster types computed for the last batch");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t n = c->h_counts[(size_t)s * 8 + 4];
    if (n > cap) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    if ((rc = merge_check(c))) return rc;
    std::vector<uint8_t> t(n ? n : 1);
    const uint8_t* src = c->rg_done ? c->rg.cls : c->A.pt_type;  // (without the stage: pt_type, whose `other` is tree)
    if (n) HIPCHK(c, hipMemcpy(t.data(), src + c->h_scan_off[s], (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) h_type[i] = t[i] == 0 ? -1 : (t[i] == 2 ? car_label : (t[i] == 3 ? building_label : tree_label));
    return n;
}

int scvod_batch_fetch_region_growing(scvod_ctx* c, int32_t s, float* h_normal_curv, int32_t* h_segment, int32_t cap) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->types_valid || !c->rg_done)
        return fail(c, SCVOD_ERR_STATE, "no region growing ran on the last clustering (scvod_set_region_growing, scvod_batch_cluster_types)");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t n = c->h_counts[(size_t)s * 8 + 4];
    if (n > cap) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", cap, n);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    const size_t o = (size_t)c->h_scan_off[s];
    if (n && h_normal_curv) HIPCHK(c, hipMemcpy(h_normal_curv, c->rg.out_nc + o, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (n && h_segment) HIPCHK(c, hipMemcpy(h_segment, c->rg.out_seg + o, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return n;
}

int scvod_batch_region_growing_stats(scvod_ctx* c, int32_t* h_out8) {
    if (!c || !h_out8) return SCVOD_ERR_INVALID;
    if (!c->types_valid) return fail(c, SCVOD_ERR_STATE, "no cluster types computed for the last batch");
    for (int k = 0; k < 8; ++k) h_out8[k] = 0;
    if (!c->rg_done) return SCVOD_OK;
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out8, c->rg.stats, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    h_out8[7] = 0;
    return SCVOD_OK;
}

int scvod_set_region_growing(scvod_ctx* c, int32_t on, int32_t k, int32_t min_segment, double smoothness_deg, float curvature_threshold,
                             double plane_fraction) {
    if (!c) return SCVOD_ERR_INVALID;
    if (k < 1 || k > 16) return fail(c, SCVOD_ERR_INVALID, "region growing: k %d outside 1..16", k);
    if (min_segment < 1) return fail(c, SCVOD_ERR_INVALID, "region growing: min_segment %d < 1", min_segment);
    if (!(smoothness_deg > 0.0 && smoothness_deg <= 90.0)) return fail(c, SCVOD_ERR_INVALID, "region growing: smoothness outside (0, 90] degrees");
    if (!(plane_fraction >= 0.0 && plane_fraction <= 1.0)) return fail(c, SCVOD_ERR_INVALID, "region growing: plane fraction outside [0, 1]");
    if (curvature_threshold != curvature_threshold) return fail(c, SCVOD_ERR_INVALID, "region growing: NaN curvature threshold");
    c->rg_on = on != 0;
    c->rg_k = k;
    c->rg_min_seg = min_segment;
    c->rg_cos = cosf((float)(smoothness_deg / 180.0 * M_PI));  // setSmoothnessThreshold(float) and validatePoint's cosf, on the host
    c->rg_curv = curvature_threshold;
    c->rg_frac = plane_fraction;
    c->rg_done = false;
    return SCVOD_OK;
}

int scvod_set_intensity_calibration(scvod_ctx* c, int32_t on, int32_t search_num, float max_intensity) {
    if (!c) return SCVOD_ERR_INVALID;
    if (search_num < 3 || search_num > 16) return fail(c, SCVOD_ERR_INVALID, "intensity calibration: search_num %d outside 3..16", search_num);
    if (!(max_intensity > 0.f)) return fail(c, SCVOD_ERR_INVALID, "intensity calibration: max_intensity must be a positive number");
    c->cal_on = on != 0;
    c->cal_k = search_num;
    c->cal_max = max_intensity;
    return SCVOD_OK;
}

int scvod_batch_fetch_intensity_calibration(scvod_ctx* c, int32_t s, float* h_normal_curv, float* h_intensity, int32_t cap) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->batch_valid || !c->cal_done)
        return fail(c, SCVOD_ERR_STATE, "no intensity calibration ran on the last batch (scvod_set_intensity_calibration before scvod_batch_process)");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    const int32_t n = c->h_counts[(size_t)s * 8 + 2];
    if (n > cap) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", cap, n);
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->last_stream;
    if (c->cal_fetch_cap < n) {  // the neighbour lists and normals never reach HBM in a batch: the scan is calibrated again for the fetch
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->cal_fetch) {
            HIPCHK(c, hipFree(c->cal_fetch));
            c->side_bytes -= c->cal_fetch_bytes;
            c->cal_fetch = nullptr;
        }
        const int64_t want = std::max<int64_t>(n, c->A.max_scan_pts);
        c->cal_fetch_bytes = align_up(sizeof(float) * 5 * (size_t)want, 256);
        HIPCHK(c, hipMalloc(&c->cal_fetch, c->cal_fetch_bytes));
        c->side_bytes += c->cal_fetch_bytes;
        c->cal_fetch_cap = want;
    }
    const int64_t pts = (int64_t)c->h_scan_off[s + 1] - c->h_scan_off[s];
    rc = ensure_calib(c, pts);
    if (rc) return rc;
    CalJob J = c->cal;
    J.k = c->cal_k;
    J.max_int = c->cal_max;
    J.write_apri = 0;
    J.force_fallback = 0;
    J.out_nc = (float4*)c->cal_fetch;
    J.out_int = (float*)((float4*)c->cal_fetch + c->cal_fetch_cap);
    J.stats = nullptr;
    J.s0 = s;
    J.ns = 1;
    J.off0 = c->h_scan_off[s];
    if (int rc_lists = ensure_lists(c, st)) return rc_lists;  // (k_cal_* walk nonground_idx; a calibrated batch emitted eagerly: a no-op today)
    launch_calib(c->A, J, (int)pts, st, nullptr, nullptr);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    if (h_normal_curv) HIPCHK(c, hipMemcpy(h_normal_curv, J.out_nc, sizeof(float4) * n, hipMemcpyDeviceToHost));
    if (h_intensity) HIPCHK(c, hipMemcpy(h_intensity, J.out_int, sizeof(float) * n, hipMemcpyDeviceToHost));
    return n;
}

int scvod_batch_intensity_calibration_stats(scvod_ctx* c, int32_t* h_out8) {
    if (!c || !h_out8) return SCVOD_ERR_INVALID;
    if (!c->batch_valid) return fail(c, SCVOD_ERR_STATE, "no batch has been run");
    for (int k = 0; k < 8; ++k) h_out8[k] = 0;
    if (!c->cal_done || c->A.max_scan_pts <= 0) return SCVOD_OK;
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out8, c->cal.stats, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    h_out8[7] = 0;
    return SCVOD_OK;
}

int scvod_batch_intensity_calibration_candidates(scvod_ctx* c, int64_t* h_out) {
    if (!c || !h_out) return SCVOD_ERR_INVALID;
    if (!c->batch_valid) return fail(c, SCVOD_ERR_STATE, "no batch has been run");
    *h_out = 0;
    if (!c->cal_done || c->A.max_scan_pts <= 0) return SCVOD_OK;
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out, c->cal.cand, sizeof(int64_t), hipMemcpyDeviceToHost));
    return SCVOD_OK;
}

int scvod_cluster(scvod_ctx* c, const scvod_apri* h_apri, int32_t n, int32_t* h_pt_cluster) {
    scvod_scan_result r;
    int rc = scvod_voxelize(c, h_apri, n, &r);
    if (rc) return rc;
    rc = scvod_batch_cluster(c, nullptr, 1);
    if (rc) return rc;
    rc = scvod_batch_fetch_clusters(c, 0, h_pt_cluster, n);
    return rc < 0 ? rc : SCVOD_OK;
}

int scvod_batch_track(scvod_ctx* c, const float* h_T, const int32_t* h_next_scan, const void* const* h_ext_tables, int32_t n_ext,
                      void* stream, int32_t sync) {
    if (!c || !h_T || n_ext < 0 || (n_ext > 0 && !h_ext_tables)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->batch_valid || !c->voxels_valid || !c->clusters_valid || !c->types_valid)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_track needs scvod_batch_process, scvod_batch_cluster and scvod_batch_cluster_types first");
    if (int rc = merge_check(c)) return rc;
    if (c->batch_mode == 3) return fail(c, SCVOD_ERR_STATE, "the last batch was a VoxelGrid run");
    const int B = c->A.n_scans;
    if (n_ext > c->cap_scans) return fail(c, SCVOD_ERR_CAPACITY, "too many external tables");
    if ((int)c->halo.size() > B)  // (a mask left over from a batch with another layout would silently turn leading scans into warm-up only)
        return fail(c, SCVOD_ERR_INVALID, "the halo mask covers %d scans, the batch holds %d: call scvod_set_track_owned / scvod_set_track_halo for this batch", (int)c->halo.size(), B);
    std::vector<int32_t> next(B);
    for (int s = 0; s < B; ++s) {
        const int32_t v = h_next_scan ? h_next_scan[s] : (s + 1 < B ? s + 1 : -1);
        if (v >= B || (v <= -2 && -2 - v >= n_ext)) return fail(c, SCVOD_ERR_INVALID, "next_scan[%d] = %d out of range", s, v);
        next[s] = v;
    }
    for (int e = 0; e < n_ext; ++e)
        if (!h_ext_tables[e]) return fail(c, SCVOD_ERR_INVALID, "external table %d is NULL", e);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    c->last_stream = st;
    c->tim_used = 0;
    int rc;
    if ((rc = upload_if_changed(c, c->up_T, h_T, (size_t)12 * B, c->t_T, st))) return rc;
    if ((rc = upload_if_changed(c, c->up_next, next.data(), (size_t)B, c->d_next_scan, st))) return rc;
    if ((rc = upload_if_changed(c, c->up_ext, h_ext_tables, (size_t)n_ext, (void*)c->d_ext, st))) return rc;
    TrackBatch J;
    J.next_scan = c->d_next_scan;
    J.ext_tables = c->d_ext;
    J.n_ext = n_ext;
    J.T = c->t_T;
    J.occupancy = c->params.occupancy;
    ChainJob CJ;
    memset(&CJ, 0, sizeof(CJ));
    c->chain_ran = false;
    if (c->track_mode == SCVOD_TRACK_CHAIN && c->A.max_scan_pts > 0) {
        std::vector<int32_t> scans, fw, walkers;
        const int nw = plan_chains(c, next, scans, fw, walkers);
        if (nw < 0) return nw;
        if (nw > 0) {
            // The layout follows the LARGEST scan this ctx has tracked so far (rounded up to 4096 points), not the current batch's:
            // a stream of batches whose largest scan wobbles keeps one layout, one workspace, and is not cleared again
            const int lay_pts = ((c->A.max_scan_pts + 4095) / 4096) * 4096;
            if (lay_pts > c->chain_geom_pts || c->chain_geom_pool != c->chain_pool_points) {
                const int pts = lay_pts > c->chain_geom_pts ? lay_pts : c->chain_geom_pts;
                chain_layout(c->chain_geom, pts, c->chain_pool_points);
                c->chain_geom_pts = pts;
                c->chain_geom_pool = c->chain_pool_points;
                c->chain_ws_clean = false;
            }
            // (the plan cut by measured time -- the stream's second or third batch -- has up to one walker per CU: room for them from the first call,
            //  or that batch would stop the device, free, allocate and clear ~18 GB again: 3.7 ms of a one-shot job's second step, round 6)
            const int nw_room = (c->chain_seg <= 0 && c->chain_balance && nw < c->n_cu) ? c->n_cu : nw;
            const size_t need = (size_t)nw_room * c->chain_geom.stride;
            if (need > c->chain_ws_bytes) {  // first call / larger job: the only allocation, outside any steady-state step
                HIPCHK(c, hipDeviceSynchronize());
                if (c->chain_ws) hipFree(c->chain_ws);
                c->chain_ws = nullptr;
                c->chain_ws_bytes = 0;
                HIPCHK(c, hipMalloc(&c->chain_ws, need));
                c->chain_ws_bytes = need;
                c->chain_ws_clean = false;
            }
            // the stamped override words compare against a per-walker epoch that only grows: a zeroed workspace is a valid one
            if (!c->chain_ws_clean || c->chain_ws_layout_pts != c->chain_geom_pts) {
                HIPCHK(c, hipMemsetAsync(c->chain_ws, 0, c->chain_ws_bytes, st));
                c->chain_ws_clean = true;
                c->chain_ws_layout_pts = c->chain_geom_pts;
            }
            if ((rc = upload_if_changed(c, c->up_chain_scans, scans.data(), scans.size(), c->d_chain_scans, st))) return rc;
            if ((rc = upload_if_changed(c, c->up_chain_fw, fw.data(), fw.size(), c->d_chain_fw, st))) return rc;
            if ((rc = upload_if_changed(c, c->up_chain_walkers, walkers.data(), walkers.size(), (void*)c->d_chain_walkers, st))) return rc;
            HIPCHK(c, hipMemsetAsync(c->d_chain_stats, 0, 8 * sizeof(int32_t), st));
            CJ.chain_scans = c->d_chain_scans;
            CJ.walkers = c->d_chain_walkers;
            CJ.chain_first_walker = c->d_chain_fw;
            CJ.n_walkers = nw;
            CJ.n_chains = (int)fw.size() - 1;
            CJ.ws = c->chain_geom;
            CJ.ws.base = (unsigned char*)c->chain_ws;
            CJ.stats = c->d_chain_stats;
            CJ.words = (c->chain_geom_pts + 31) / 32 + 1;  // (sized like the layout: one value for the workspace and the bitsets)
            const size_t lds_bits = 72 * 1024;  // next to the 80 KB of per-step tables
            int ev = (int)(lds_bits / ((size_t)CJ.words * 4));
            CJ.n_eval_waves = ev < 1 ? 1 : (ev > 16 ? 16 : ev);
            if ((size_t)CJ.words * 4 > lds_bits) return fail(c, SCVOD_ERR_CAPACITY, "scan too large for the chain's LDS bitset");
            CJ.force_generic = c->chain_generic ? 1 : 0;
            CJ.literal_max_name = (c->max_name_literal && c->last_name_valid) ? 1 : 0;
            CJ.ext_state = nullptr;
            CJ.resume = 0;
            CJ.step_ticks = c->d_step_ticks;
            HIPCHK(c, hipMemsetAsync(c->d_step_ticks, 0, sizeof(int32_t) * scans.size(), st));
            c->plan_scans_tmp = scans;
            c->last_cj = CJ;
            c->last_tb = J;
            c->chain_ran = true;
        }
    }
    launch_track_batch(c->dev, c->A, J, c->batch_mode == 2 ? 1 : 0, c->tables_valid ? 2 : 3, st, timer_hook, c, c->chain_ran ? &CJ : nullptr,
                       c->ln_pending ? c->ln_done : nullptr);
    if (c->chain_ran) c->ln_pending = false;  // (the chain waited for it)
    if (c->chain_ran) {  // the counters of this chain, for the warm-up of the stream's next batch
        if (!c->h_chain_fb) {
            HIPCHK(c, hipHostMalloc((void**)&c->h_chain_fb, 8 * sizeof(int32_t)));
            HIPCHK(c, hipEventCreateWithFlags(&c->chain_fb_ev, hipEventDisableTiming));
        }
        if (!c->chain_fb_pending) {
            HIPCHK(c, hipMemcpyAsync(c->h_chain_fb, c->d_chain_stats, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipEventRecord(c->chain_fb_ev, st));
            c->chain_fb_pending = true;
            c->chain_fb_segments = CJ.n_walkers;
        }
        if (!c->h_step_ticks) {
            HIPCHK(c, hipHostMalloc((void**)&c->h_step_ticks, sizeof(int32_t) * (size_t)(c->cap_scans + 1)));
            HIPCHK(c, hipEventCreateWithFlags(&c->step_fb_ev, hipEventDisableTiming));
        }
        if (!c->step_fb_pending && c->chain_balance && !(c->cuts_scans == c->plan_scans_tmp && !c->cuts_cache.empty())) {  // the per-step times, for the cuts of the stream's next batch
            HIPCHK(c, hipMemcpyAsync(c->h_step_ticks, c->d_step_ticks, sizeof(int32_t) * c->plan_scans_tmp.size(), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipEventRecord(c->step_fb_ev, st));
            c->step_fb_pending = true;
            c->step_fb_scans = c->plan_scans_tmp;
        }
    }
    HIPCHK(c, hipGetLastError());
    c->tables_valid = true;
    c->track_valid = true;
    if (sync) HIPCHK(c, hipStreamSynchronize(st));
    return SCVOD_OK;
}

int scvod_get_params(const scvod_ctx* c, scvod_params* out) {
    if (!c || !out) return SCVOD_ERR_INVALID;
    *out = c->params;
    return SCVOD_OK;
}

int64_t scvod_chain_workspace_bytes(scvod_ctx* c) { return c ? (int64_t)c->chain_ws_bytes : 0; }

int scvod_set_track_owned(scvod_ctx* c, int32_t first_owned_scan) {
    if (!c || first_owned_scan < 0) return fail(c, SCVOD_ERR_INVALID, "bad first owned scan");
    c->halo.assign((size_t)first_owned_scan, 1);
    c->track_valid = false;
    return SCVOD_OK;
}

int scvod_set_track_halo(scvod_ctx* c, const uint8_t* h_is_halo, int32_t n_scans) {
    if (!c || n_scans < 0 || (n_scans > 0 && !h_is_halo)) return fail(c, SCVOD_ERR_INVALID, "bad halo mask");
    c->halo.assign(h_is_halo, h_is_halo + n_scans);
    c->track_valid = false;
    return SCVOD_OK;
}

int64_t scvod_chain_state_bytes(scvod_ctx* c) {
    if (!c || !c->chain_ran) return 0;
    return (int64_t)chain_state_bytes(c->last_cj.ws);
}

int scvod_chain_export_state(scvod_ctx* c, int32_t chain, int32_t which, void* d_dst, int64_t cap_bytes, void* stream) {
    if (!c || !d_dst || (which != 0 && which != 1)) return SCVOD_ERR_INVALID;
    if (!c->track_valid || !c->chain_ran) return fail(c, SCVOD_ERR_STATE, "no tracking chain of the last batch");
    if (chain < 0 || chain >= c->last_cj.n_chains) return fail(c, SCVOD_ERR_INVALID, "chain %d out of range (%d chains)", chain, c->last_cj.n_chains);
    if (cap_bytes < 16) return fail(c, SCVOD_ERR_CAPACITY, "state buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);  // (behind the walkers of the last scvod_batch_track)
    launch_chain_export_state(c->last_cj, chain, which, (unsigned char*)d_dst, cap_bytes, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

int scvod_batch_track_chains(scvod_ctx* c, int32_t* h_first_scan, int32_t cap) {
    if (!c || !h_first_scan) return SCVOD_ERR_INVALID;
    if (!c->track_valid || !c->chain_ran) return fail(c, SCVOD_ERR_STATE, "no tracking chain of the last batch");
    const int nc = c->last_cj.n_chains;
    if (cap < nc) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d chains)", cap, nc);
    // a chain without a step of its own has no walker: its head is reported all the same (up_chain_fw / up_chain_scans hold the plan)
    int k = 0;
    std::vector<char> is_succ(c->up_next.size(), 0);
    for (size_t s = 0; s < c->up_next.size(); ++s)
        if (c->up_next[s] >= 0) is_succ[c->up_next[s]] = 1;
    for (size_t s = 0; s < c->up_next.size() && k < nc; ++s)
        if (!is_succ[s] && c->up_next[s] >= 0) h_first_scan[k++] = (int32_t)s;
    return nc;
}

int scvod_batch_track_resume(scvod_ctx* c, const void* const* h_d_states, int32_t n_states, void* stream, int32_t sync) {
    if (!c || !h_d_states) return SCVOD_ERR_INVALID;
    if (!c->track_valid || !c->chain_ran) return fail(c, SCVOD_ERR_STATE, "scvod_batch_track_resume needs a chain-mode scvod_batch_track first");
    if (n_states != c->last_cj.n_chains) return fail(c, SCVOD_ERR_INVALID, "%d states for %d chains", n_states, c->last_cj.n_chains);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    c->last_stream = st;
    c->ext_state_pin_valid = false;
    HIPCHK(c, hipMemcpyAsync((void*)c->d_ext_state, h_d_states, sizeof(void*) * (size_t)n_states, hipMemcpyHostToDevice, st));
    ChainJob CJ = c->last_cj;
    CJ.ext_state = c->d_ext_state;
    CJ.resume = 1;
    launch_track_chain_resume(c->dev, c->A, c->last_tb, CJ, c->batch_mode == 2 ? 1 : 0, st);
    launch_track_dyn(c->A, c->batch_mode == 2 ? 1 : 0, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));  // (the pointer table is a pageable host array)
    (void)sync;
    return SCVOD_OK;
}

int scvod_batch_track_compare(scvod_ctx* c, const void* const* h_d_states, int32_t n_states, int32_t* h_differ, void* stream) {
    if (!c || !h_d_states || !h_differ) return SCVOD_ERR_INVALID;
    if (!c->track_valid || !c->chain_ran) return fail(c, SCVOD_ERR_STATE, "scvod_batch_track_compare needs a chain-mode scvod_batch_track first");
    if (n_states != c->last_cj.n_chains) return fail(c, SCVOD_ERR_INVALID, "%d states for %d chains", n_states, c->last_cj.n_chains);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    c->last_stream = st;
    c->ext_state_pin_valid = false;
    HIPCHK(c, hipMemcpyAsync((void*)c->d_ext_state, h_d_states, sizeof(void*) * (size_t)n_states, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(c->d_chain_cmp, 0, sizeof(int32_t), st));
    ChainJob CJ = c->last_cj;
    CJ.ext_state = c->d_ext_state;
    CJ.resume = 2;
    CJ.cmp_out = c->d_chain_cmp;
    launch_track_chain_resume(c->dev, c->A, c->last_tb, CJ, c->batch_mode == 2 ? 1 : 0, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_differ, c->d_chain_cmp, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return SCVOD_OK;
}

int scvod_batch_track_compare_device(scvod_ctx* c, const void* const* h_d_states, int32_t n_states, int32_t* d_differ, void* stream) {
    if (!c || !h_d_states || !d_differ) return SCVOD_ERR_INVALID;
    if (!c->track_valid || !c->chain_ran) return fail(c, SCVOD_ERR_STATE, "scvod_batch_track_compare_device needs a chain-mode scvod_batch_track first");
    if (n_states != c->last_cj.n_chains) return fail(c, SCVOD_ERR_INVALID, "%d states for %d chains", n_states, c->last_cj.n_chains);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    c->last_stream = st;
    // the pointer table goes through a pinned copy of the ctx (nothing waits on the host, the caller's array may go away); it is
    // uploaded again only when it changed (a shard's receive buffers stay where they are from step to step)
    if (!c->h_ext_state_pin) HIPCHK(c, hipHostMalloc((void**)&c->h_ext_state_pin, sizeof(void*) * (size_t)c->cap_scans));
    if (!c->ext_state_pin_valid || c->ext_state_pin_n != n_states || memcmp(c->h_ext_state_pin, h_d_states, sizeof(void*) * (size_t)n_states) != 0) {
        if (c->ext_state_pin_valid) HIPCHK(c, hipStreamSynchronize(st));  // (a table in flight is still being read: rare, the table changed)
        memcpy(c->h_ext_state_pin, h_d_states, sizeof(void*) * (size_t)n_states);
        HIPCHK(c, hipMemcpyAsync((void*)c->d_ext_state, c->h_ext_state_pin, sizeof(void*) * (size_t)n_states, hipMemcpyHostToDevice, st));
        c->ext_state_pin_valid = true;
        c->ext_state_pin_n = n_states;
    }
    ChainJob CJ = c->last_cj;
    CJ.ext_state = c->d_ext_state;
    CJ.resume = 2;
    CJ.cmp_out = d_differ;
    launch_track_chain_resume(c->dev, c->A, c->last_tb, CJ, c->batch_mode == 2 ? 1 : 0, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

int scvod_set_cluster_exact(scvod_ctx* c, int32_t on) {
    if (!c) return SCVOD_ERR_INVALID;
    c->A.cc_exact_max = on ? 0x3fffffff : 4096;
    c->A.cc_plain_rule = on == 2 ? 0 : 1;
    c->A.cc_help_blocks_wanted = on == 3 ? 0 : 1;  // 3: exact, every scan's workgroup on its own (the round-5 form: A/B runs, tests of the shared rounds)
    c->clusters_valid = c->types_valid = c->tables_valid = c->track_valid = false;
    return SCVOD_OK;
}

int scvod_batch_cluster_stats(scvod_ctx* c, int32_t* h_out4) {
    if (!c || !h_out4) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "no clustering of the last batch");
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out4, c->A.cc_stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    h_out4[2] = c->A.cc_exact_max > 4096 ? 1 : 0;
    return SCVOD_OK;
}

int scvod_batch_cluster_rule_stats(scvod_ctx* c, int32_t* h_out2) {
    if (!c || !h_out2) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "no clustering of the last batch");
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out2, c->A.cc_stats + 4, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SCVOD_OK;
}

int scvod_batch_cluster_help_stats(scvod_ctx* c, int32_t* h_out2) {
    if (!c || !h_out2) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "no clustering of the last batch");
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out2, c->A.cc_help, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(h_out2 + 1, c->A.cc_stats + 6, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (getenv("SCVOD_CC_HELP_DUMP")) {  // development: the board of the last launch (10 ns ticks relative to the first scan block)
        std::vector<int32_t> b(kCcHelpWords);
        HIPCHK(c, hipMemcpy(b.data(), c->A.cc_help, b.size() * 4, hipMemcpyDeviceToHost));
        auto t64 = [&](size_t w) { return *reinterpret_cast<long long*>(&b[w]); };
        long long t0 = 0x7fffffffffffffffll;
        for (int k = 0; k < b[0] && k < kCcHelpSlots; ++k) t0 = std::min(t0, t64(kCcHelpHdr + (size_t)k * kCcHelpSlotWords + 20));
        int32_t nr = 0;
        HIPCHK(c, hipMemcpy(&nr, c->A.cc_again, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "cc_help: %d scans handed to k_cc_exact, %d asked for help, %d past their shared passes (clocks: x10 ns after the first rounds began)\n", nr, b[0], b[1]);
        for (int k = 0; k < b[0] && k < kCcHelpSlots; ++k) {
            const size_t w = kCcHelpHdr + (size_t)k * kCcHelpSlotWords;
            fprintf(stderr, "  slot %d scan %d: na %d chunks/round %d rounds %d leader chunks %d | entry +%lld rule done +%lld listed +%lld rounds start +%lld end +%lld unions end +%lld scan done +%lld\n", k, b[w + 18], b[w + 3], b[w + 4], b[w + 19], b[w + 5],
                    t64(w + 38) - t0, t64(w + 40) - t0, t64(w + 42) - t0, t64(w + 20) - t0, t64(w + 22) - t0, t64(w + 24) - t0, t64(w + 54) - t0);
        }
    }
    return SCVOD_OK;
}

int scvod_set_intensity_merge(scvod_ctx* c, int32_t iterations, int32_t search_c, float intensity_diff, float intensity_cov) {
    if (!c) return SCVOD_ERR_INVALID;
    if (iterations < 0 || !(intensity_diff >= 0.f) || !(intensity_cov >= 0.f))
        return fail(c, SCVOD_ERR_INVALID, "intensity merge: negative parameter");
    if (search_c < 1 || search_c > 3)
        return fail(c, SCVOD_ERR_INVALID, "intensity merge: search_c %d outside 1..3", search_c);
    c->im_iterations = iterations;
    c->im_search_c = search_c;
    c->im_diff = intensity_diff;
    c->im_cov = intensity_cov;
    c->clusters_valid = c->types_valid = c->tables_valid = c->track_valid = false;
    return SCVOD_OK;
}

int scvod_set_voxel_descriptors(scvod_ctx* c, int32_t mode) {
    if (!c) return SCVOD_ERR_INVALID;
    if (mode != 0 && mode != 1) return fail(c, SCVOD_ERR_INVALID, "voxel descriptors: mode %d is neither 0 (on demand) nor 1 (eager)", mode);
    c->desc_mode = mode;  // (takes effect with the next batch; the current one keeps what it has)
    return SCVOD_OK;
}

int scvod_batch_cluster_merge_stats(scvod_ctx* c, int32_t* h_out4) {
    if (!c || !h_out4) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid) return fail(c, SCVOD_ERR_STATE, "no clustering of the last batch");
    for (int k = 0; k < 4; ++k) h_out4[k] = 0;
    if (!c->merged) return SCVOD_OK;
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    int32_t st[8];
    HIPCHK(c, hipMemcpy(st, c->im.stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) h_out4[k] = st[k];
    return merge_check(c);
}

int scvod_set_max_name_literal(scvod_ctx* c, int32_t literal) {
    if (!c) return SCVOD_ERR_INVALID;
    c->max_name_literal = literal != 0;
    c->clusters_valid = c->types_valid = c->tables_valid = c->track_valid = false;  // (the clustering publishes the name)
    return SCVOD_OK;
}

int scvod_batch_cluster_last_name(scvod_ctx* c, int32_t* h_out4, int32_t cap_scans, int32_t* h_stats4) {
    if (!c || !h_out4) return SCVOD_ERR_INVALID;
    if (!c->clusters_valid || !c->last_name_valid) return fail(c, SCVOD_ERR_STATE, "no clustering with max_name tracking for the last batch");
    if (cap_scans < c->A.n_scans) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d scans)", cap_scans, c->A.n_scans);
    join_lastname(c, c->last_stream);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(h_out4, c->A.cc_last, sizeof(int32_t) * 4 * (size_t)c->A.n_scans, hipMemcpyDeviceToHost));
    if (h_stats4) HIPCHK(c, hipMemcpy(h_stats4, c->A.ln_stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (getenv("SCVOD_LN_PROF")) {  // development: phase clocks of the first scans
        std::vector<int32_t> pr(8 * (size_t)c->A.n_scans);
        HIPCHK(c, hipMemcpy(pr.data(), c->A.ln_prof, pr.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int32_t> pr2(pr.size());
        HIPCHK(c, hipMemcpy(pr2.data(), c->A.ln_prof2, pr2.size() * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < c->A.n_scans && s < 64; ++s)
            fprintf(stderr, "ln_big scan %d: nodes %d rounds %d build %d jacobi %d open %d cc %d walk %d events %d\n", s, pr2[8 * s], pr2[8 * s + 1], pr2[8 * s + 2], pr2[8 * s + 3], pr2[8 * s + 4], pr2[8 * s + 5], pr2[8 * s + 6], pr2[8 * s + 7]),
            fprintf(stderr, "ln_prof scan %d: setup %d A+irr.. CL %d cand %d marked %d (x10ns) n_cand %d n_mk %d n_irr %d cap %d\n", s, pr[8 * s], pr[8 * s + 1], pr[8 * s + 2], pr[8 * s + 3], pr[8 * s + 4], pr[8 * s + 5], pr[8 * s + 6], pr[8 * s + 7]);
    }
    return c->A.n_scans;
}

int scvod_set_chain_capacity(scvod_ctx* c, int64_t pool_points) {
    if (!c || pool_points < 0 || pool_points > (1ll << 30)) return fail(c, SCVOD_ERR_INVALID, "bad chain capacity");
    c->chain_pool_points = pool_points;
    return SCVOD_OK;
}

int scvod_set_track_mode(scvod_ctx* c, int32_t mode, int32_t segment_steps, int32_t warmup_steps) {
    if (!c || (mode != SCVOD_TRACK_CHAIN && mode != SCVOD_TRACK_FIRST_ORDER && mode != SCVOD_TRACK_CHAIN_GENERIC))
        return fail(c, SCVOD_ERR_INVALID, "unknown tracking mode");
    if (segment_steps < 0 || warmup_steps < -1) return fail(c, SCVOD_ERR_INVALID, "negative segment / warm-up length");
    c->chain_generic = (mode == SCVOD_TRACK_CHAIN_GENERIC);
    if (mode == SCVOD_TRACK_CHAIN_GENERIC) mode = SCVOD_TRACK_CHAIN;
    c->track_mode = mode;
    c->chain_seg = segment_steps;                   // 0: chosen per job
    if (warmup_steps >= 0) c->chain_warm = warmup_steps;  // -1: keep
    c->track_valid = false;
    return SCVOD_OK;
}

// error bits / counters of the chain of the last scvod_batch_track (synchronises its stream)
static int chain_status(scvod_ctx* c, int32_t out[8]) {
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!c->chain_ran) return SCVOD_OK;
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    HIPCHK(c, hipMemcpy(out, c->d_chain_stats, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out[0])
        return fail(c, SCVOD_ERR_CAPACITY, "tracking chain overflow (bits %d: 1 appended clouds > %d points (scvod_set_chain_capacity), 2 more than %d clusters, 4 created labels, 8 table > bitset)",
                    out[0], c->chain_geom.cap_pool, c->chain_geom.cap_ent);
    return SCVOD_OK;
}

int scvod_batch_track_stats(scvod_ctx* c, int32_t* h_out8) {
    if (!c || !h_out8) return SCVOD_ERR_INVALID;
    if (!c->track_valid) return fail(c, SCVOD_ERR_STATE, "no tracking result for the last batch");
    int32_t st[8];
    const int rc = chain_status(c, st);
    h_out8[0] = c->chain_ran ? SCVOD_TRACK_CHAIN : SCVOD_TRACK_FIRST_ORDER;
    h_out8[1] = (int32_t)(c->up_chain_walkers.size() / 8) * (c->chain_ran ? 1 : 0);
    h_out8[2] = st[2];
    h_out8[3] = st[1];
    h_out8[4] = st[0];
    h_out8[5] = c->chain_seg_used;
    h_out8[6] = c->chain_warm_used;
    h_out8[7] = 0;
    if (c->chain_ran && c->max_name_literal && c->last_name_valid) {  // scans whose max_name the clustering could not determine: the chain handed out a fresh number there
        int32_t ls[4] = {0, 0, 0, 0};
        HIPCHK(c, hipMemcpy(ls, c->A.ln_stats, sizeof(ls), hipMemcpyDeviceToHost));
        h_out8[7] = ls[0] + ls[1];
    }
#ifdef SCVOD_PROFILE
    fprintf(stderr, "[chain phases, 10 ns ticks summed over walkers x steps] fetch %d  carried %d  eval %d  walk+state %d  copy %d\n", st[3], st[4], st[5], st[6], st[7]);
    if (c->chain_ran) {
        const int nw = (int)(c->up_chain_walkers.size() / 8);
        std::vector<int32_t> hd(16);
        long long sum = 0;
        int mn = 0x7fffffff, mx = 0;
        std::vector<int> all;
        for (int w = 0; w < nw; ++w) {
            hipMemcpy(hd.data(), (unsigned char*)c->chain_ws + (size_t)w * c->chain_geom.stride + c->chain_geom.off_hdr, 64, hipMemcpyDeviceToHost);
            sum += hd[15];
            mn = hd[15] < mn ? hd[15] : mn;
            mx = hd[15] > mx ? hd[15] : mx;
            all.push_back(hd[15]);
        }
        std::sort(all.begin(), all.end());
        fprintf(stderr, "[chain walkers] %d: wall min %.1f us  median %.1f  p90 %.1f  max %.1f  mean %.1f\n", nw, mn * 0.01, all[nw / 2] * 0.01, all[nw * 9 / 10] * 0.01,
                mx * 0.01, sum * 0.01 / nw);
    }
#endif
    return rc;
}

int scvod_batch_track_tables(scvod_ctx* c, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->batch_valid || !c->voxels_valid || !c->clusters_valid || !c->types_valid)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_track_tables needs scvod_batch_process, scvod_batch_cluster and scvod_batch_cluster_types first");
    if (int rc = merge_check(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    c->last_stream = st;
    join_lastname(c, st);
    c->tim_used = 0;
    TrackBatch J;
    memset(&J, 0, sizeof(J));
    launch_track_batch(c->dev, c->A, J, 0, 1, st, timer_hook, c);
    HIPCHK(c, hipGetLastError());
    c->tables_valid = true;
    c->track_valid = false;
    return SCVOD_OK;
}

int scvod_batch_export_table(scvod_ctx* c, int32_t s, void* d_out, int64_t cap_records, void* stream) {
    if (!c || !d_out || cap_records < 1) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->tables_valid) return fail(c, SCVOD_ERR_STATE, "scvod_batch_export_table needs scvod_batch_track_tables or scvod_batch_track first");
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    launch_export_table(c->A, s, (int4*)d_out, (long long)cap_records, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

int scvod_batch_fetch_track(scvod_ctx* c, int32_t s, scvod_track_result* out) {
    if (!c || !out) return SCVOD_ERR_INVALID;
    if (!c->track_valid) return fail(c, SCVOD_ERR_STATE, "no tracking result for the last batch");
    int rc = ensure_counts(c);
    if (rc) return rc;
    if (s < 0 || s >= c->A.n_scans) return fail(c, SCVOD_ERR_INVALID, "scan %d out of range", s);
    HIPCHK(c, hipStreamSynchronize(c->last_stream));
    {
        int32_t cst[8];
        if ((rc = chain_status(c, cst))) return rc;
    }
    const Arena& A = c->A;
    const size_t base = (size_t)c->h_scan_off[s];
    const int n = c->h_counts[(size_t)s * 8 + 4];
    int32_t sc[4];
    HIPCHK(c, hipMemcpy(sc, A.tk_scan + (size_t)s * 4, sizeof(sc), hipMemcpyDeviceToHost));
    const int ncl = sc[0] < 0 ? 0 : (sc[0] > n ? n : sc[0]);
    memset(out, 0, sizeof(*out));
    out->n_apri = n;
    out->n_clusters = ncl;
    out->n_car_points = sc[1];
    out->n_dynamic_clusters = sc[2];
    out->n_dynamic_points = sc[3];
    // per-root device arrays of this scan -> compact per-cluster host arrays
    const size_t nn = n > 0 ? (size_t)n : 1;
    std::vector<int32_t> roots(nn), cnt(nn), nuq(nn), npr(nn), mbeg(nn);
    std::vector<int8_t> state(nn);
    std::vector<int2> pairs(nn);
    c->tk_stage_dyn.resize(nn);
    if (n) {
        HIPCHK(c, hipMemcpy(roots.data(), A.tk_clusters + base, 4 * (size_t)(ncl > 0 ? ncl : 0), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(cnt.data(), A.cl_count + base, 4 * nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(nuq.data(), A.tk_nuniq + base, 4 * nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(npr.data(), A.tk_npairs + base, 4 * nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(mbeg.data(), A.tk_mbegin + base, 4 * nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(state.data(), A.cl_state + base, nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(pairs.data(), A.tk_pairs + base, 8 * nn, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->tk_stage_dyn.data(), A.pt_dyn + base, nn, hipMemcpyDeviceToHost));
    }
    size_t n_pairs = 0;
    for (int k = 0; k < ncl; ++k) n_pairs += (size_t)npr[roots[k]];
    std::vector<int32_t>& h = c->tk_stage;
    h.assign((size_t)5 * ncl + 1 + 2 * n_pairs + 8, 0);
    int32_t* p_root = h.data();
    int32_t* p_size = p_root + ncl;
    int32_t* p_state = p_size + ncl;
    int32_t* p_nuq = p_state + ncl;
    int32_t* p_pbeg = p_nuq + ncl;
    int32_t* p_plab = p_pbeg + ncl + 1;
    int32_t* p_pcnt = p_plab + n_pairs;
    size_t o = 0;
    for (int k = 0; k < ncl; ++k) {
        const int r = roots[k];
        p_root[k] = r;
        p_size[k] = cnt[r];
        p_state[k] = state[r];
        p_nuq[k] = nuq[r];
        p_pbeg[k] = (int32_t)o;
        for (int j = 0; j < npr[r]; ++j, ++o) {
            p_plab[o] = pairs[(size_t)mbeg[r] + j].x;
            p_pcnt[o] = pairs[(size_t)mbeg[r] + j].y;
        }
    }
    p_pbeg[ncl] = (int32_t)o;
    out->cluster_root = p_root;
    out->cluster_size = p_size;
    out->cluster_state = p_state;
    out->n_unique = p_nuq;
    out->pair_begin = p_pbeg;
    out->pair_label = p_plab;
    out->pair_count = p_pcnt;
    out->pt_dyn = c->tk_stage_dyn.data();
    return SCVOD_OK;
}

// ---- the result handed on: per-input-point labels and the kept points of the batch (scvod_export.hip) ----
// what both calls need of the ctx: a Patchwork batch, its clustering and types, and -- unless the dynamic points are ignored -- a
// tracking result that is current (the test scvod_batch_map_accumulate applies)
static int export_check(scvod_ctx* c, int use_dyn, const char* who) {
    if (!c->batch_valid || c->batch_mode != 1 || !c->A.pts) return fail(c, SCVOD_ERR_STATE, "%s needs a batch of scvod_batch_process", who);
    if (!c->clusters_valid || !c->types_valid) return fail(c, SCVOD_ERR_STATE, "%s needs scvod_batch_cluster and scvod_batch_cluster_types of the batch", who);
    if (use_dyn && !c->track_valid) return fail(c, SCVOD_ERR_INVALID, "%s: no current tracking result: run scvod_batch_track or pass SCVOD_MAP_IGNORE_DYNAMIC", who);
    return merge_check(c);
}

int scvod_batch_point_labels(scvod_ctx* c, uint8_t* d_labels, int64_t cap, int32_t flags, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!d_labels || cap < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (flags & ~SCVOD_MAP_IGNORE_DYNAMIC) return fail(c, SCVOD_ERR_INVALID, "scvod_batch_point_labels takes SCVOD_MAP_IGNORE_DYNAMIC only (flags %d)", flags);
    const int use_dyn = (flags & SCVOD_MAP_IGNORE_DYNAMIC) ? 0 : 1;
    if (int rc = export_check(c, use_dyn, "scvod_batch_point_labels")) return rc;
    if (cap < c->A.total_pts) return fail(c, SCVOD_ERR_CAPACITY, "label buffer too small (%lld < %lld points)", (long long)cap, (long long)c->A.total_pts);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    if (c->A.total_pts > 0) {
        HIPCHK(c, hipMemsetAsync(d_labels, SCVOD_PT_DROPPED, (size_t)c->A.total_pts, st));
        if (int rc = ensure_lists(c, st)) return rc;
        launch_point_labels(c->A, d_labels, use_dyn, st);
        HIPCHK(c, hipGetLastError());
    }
    return SCVOD_OK;
}

int scvod_batch_point_classes(scvod_ctx* c, uint8_t* d_classes, int64_t cap, int32_t flags, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!d_classes || cap < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (flags & ~SCVOD_MAP_IGNORE_DYNAMIC) return fail(c, SCVOD_ERR_INVALID, "scvod_batch_point_classes takes SCVOD_MAP_IGNORE_DYNAMIC only (flags %d)", flags);
    const int use_dyn = (flags & SCVOD_MAP_IGNORE_DYNAMIC) ? 0 : 1;
    if (int rc = export_check(c, use_dyn, "scvod_batch_point_classes")) return rc;
    if (cap < c->A.total_pts) return fail(c, SCVOD_ERR_CAPACITY, "class buffer too small (%lld < %lld points)", (long long)cap, (long long)c->A.total_pts);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    if (c->A.total_pts > 0) {
        HIPCHK(c, hipMemsetAsync(d_classes, SCVOD_PT_DROPPED, (size_t)c->A.total_pts, st));
        if (int rc = ensure_lists(c, st)) return rc;
        if (c->rg_done)
            launch_point_classes(c->A, c->rg.cls, d_classes, use_dyn, st);
        else
            launch_point_labels(c->A, d_classes, use_dyn, st);  // (without the stage every non-car cluster is tree: no point gets 7)
        HIPCHK(c, hipGetLastError());
    }
    return SCVOD_OK;
}

int scvod_batch_export_points(scvod_ctx* c, int32_t flags, const float* h_poses, const uint32_t* d_payload_in, void* d_xyzi_out,
                              uint32_t* d_payload_out, int32_t* d_src_out, int64_t cap_points, int32_t* d_out_offsets, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (cap_points < 0 || !d_out_offsets) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (flags & ~(SCVOD_MAP_NO_GROUND | SCVOD_MAP_NO_REJECTED | SCVOD_MAP_IGNORE_DYNAMIC))
        return fail(c, SCVOD_ERR_INVALID, "scvod_batch_export_points takes SCVOD_MAP_NO_GROUND, SCVOD_MAP_NO_REJECTED and SCVOD_MAP_IGNORE_DYNAMIC only (flags %d)", flags);
    if (d_payload_out && !d_payload_in) return fail(c, SCVOD_ERR_INVALID, "a payload output needs a payload input");
    const int use_dyn = (flags & SCVOD_MAP_IGNORE_DYNAMIC) ? 0 : 1;
    if (int rc = export_check(c, use_dyn, "scvod_batch_export_points")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    const int B = c->A.n_scans;
    if (!c->exp_labels) {  // first export of this ctx
        HIPCHK(c, hipMalloc(&c->exp_labels, (size_t)(c->cap_pts > 0 ? c->cap_pts : 1)));
        HIPCHK(c, hipMalloc(&c->exp_scan_cnt, sizeof(int32_t) * (size_t)c->cap_scans));
        HIPCHK(c, hipMalloc(&c->exp_pose, sizeof(float) * 12 * (size_t)c->cap_scans));
        HIPCHK(c, hipMalloc(&c->exp_stats, sizeof(long long) * 4));
    }
    const int tps = (c->A.max_scan_pts + kExpTile - 1) / kExpTile;
    const size_t tiles = (size_t)B * (size_t)tps;
    if (tiles > c->exp_tiles_cap) {  // (a batch with more tiles than any before: the old table may still be read by an export in flight)
        if (c->exp_tiles) {
            HIPCHK(c, hipStreamSynchronize(c->exp_stream));
            hipFree(c->exp_tiles);
            c->exp_tiles = nullptr;
            c->exp_tiles_cap = 0;
        }
        HIPCHK(c, hipMalloc(&c->exp_tiles, sizeof(int32_t) * (tiles + tiles / 2)));
        c->exp_tiles_cap = tiles + tiles / 2;
    }
    if (h_poses) {  // pcl::getTransformation per scan, staged before the call returns: h_poses is the caller's again at once
        std::vector<float> T((size_t)12 * B);
        for (int s = 0; s < B; ++s) scvod_pose_matrix(h_poses + 6 * s, T.data() + 12 * s);
        if (int rc = upload_if_changed(c, c->exp_up_pose, T.data(), T.size(), c->exp_pose, st)) return rc;
    }
    if (c->A.total_pts > 0) {
        HIPCHK(c, hipMemsetAsync(c->exp_labels, SCVOD_PT_DROPPED, (size_t)c->A.total_pts, st));
        if (int rc = ensure_lists(c, st)) return rc;
        launch_point_labels(c->A, c->exp_labels, use_dyn, st);
    }
    ExportJob J;
    J.labels = c->exp_labels;
    J.keep_mask = (1u << SCVOD_PT_UNCLUSTERED) | (1u << SCVOD_PT_STATIC_OTHER) | (1u << SCVOD_PT_STATIC_CAR);
    if (!(flags & SCVOD_MAP_NO_GROUND)) J.keep_mask |= 1u << SCVOD_PT_GROUND;
    if (!(flags & SCVOD_MAP_NO_REJECTED)) J.keep_mask |= 1u << SCVOD_PT_REJECTED;
    if (!use_dyn) J.keep_mask |= 1u << SCVOD_PT_DYNAMIC;  // (no label says DYNAMIC then: the bit only states the rule)
    J.pose = h_poses ? c->exp_pose : nullptr;
    J.payload_in = d_payload_in;
    J.out = (float4*)d_xyzi_out;
    J.payload_out = d_payload_out;
    J.src_out = d_src_out;
    J.cap = (long long)cap_points;
    J.out_off = d_out_offsets;
    J.tile_cnt = c->exp_tiles;
    J.scan_cnt = c->exp_scan_cnt;
    J.stats = c->exp_stats;
    J.tiles_per_scan = tps;
    launch_export(c->A, J, st);
    HIPCHK(c, hipGetLastError());
    c->exp_stream = st;
    c->exp_ran = true;
    return SCVOD_OK;
}

int scvod_batch_export_stats(scvod_ctx* c, int64_t* h_out4) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out4) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->exp_ran) return fail(c, SCVOD_ERR_STATE, "no scvod_batch_export_points on this ctx yet");
    HIPCHK(c, hipSetDevice(c->device));
    long long h[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->exp_stats, sizeof(h), hipMemcpyDeviceToHost, c->exp_stream));
    HIPCHK(c, hipStreamSynchronize(c->exp_stream));
    for (int k = 0; k < 4; ++k) h_out4[k] = (int64_t)h[k];
    if (h[2]) return fail(c, SCVOD_ERR_CAPACITY, "the last export kept %lld points, its buffers hold %lld", h[1], h[0]);
    return SCVOD_OK;
}

// ---- the clusters of the batch as an object table (scvod_objects.hip) ----
int scvod_batch_objects(scvod_ctx* c, int32_t flags, void* d_objects, int64_t cap_objects, int32_t* d_obj_offsets, int32_t* d_member_src,
                        int64_t cap_members, int32_t* d_point_object, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (cap_objects < 0 || cap_members < 0 || !d_obj_offsets) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (flags & ~SCVOD_OBJ_NO_TRACK) return fail(c, SCVOD_ERR_INVALID, "scvod_batch_objects takes SCVOD_OBJ_NO_TRACK only (flags %d)", flags);
    const int use_track = (flags & SCVOD_OBJ_NO_TRACK) ? 0 : 1;
    if (int rc = export_check(c, use_track, "scvod_batch_objects")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    const int B = c->A.n_scans;
    const size_t N = (size_t)(c->cap_pts > 0 ? c->cap_pts : 1);
    if (!c->obj_stats) {  // first call of this ctx
        HIPCHK(c, hipMalloc(&c->obj_scan_cnt, sizeof(int32_t) * 2 * (size_t)c->cap_scans));
        HIPCHK(c, hipMalloc(&c->obj_stats, sizeof(long long) * 4));
        c->obj_bytes += (int64_t)(sizeof(int32_t) * 2 * (size_t)c->cap_scans + sizeof(long long) * 4);
    }
    const int tps = (c->A.max_scan_pts + kExpTile - 1) / kExpTile;
    const size_t tiles = (size_t)B * (size_t)tps;
    if (tiles > c->obj_tiles_cap) {  // (the old table may still be read by a call in flight)
        if (c->obj_tiles) {
            HIPCHK(c, hipStreamSynchronize(c->obj_stream));
            hipFree(c->obj_tiles);
            c->obj_tiles = nullptr;
            c->obj_bytes -= (int64_t)(sizeof(int32_t) * 2 * c->obj_tiles_cap);
            c->obj_tiles_cap = 0;
        }
        HIPCHK(c, hipMalloc(&c->obj_tiles, sizeof(int32_t) * 2 * (tiles + tiles / 2)));
        c->obj_tiles_cap = tiles + tiles / 2;
        c->obj_bytes += (int64_t)(sizeof(int32_t) * 2 * c->obj_tiles_cap);
    }
    const bool lists = d_objects || d_member_src || d_point_object;
    if (lists && !c->obj_keys) {  // first call that asks for more than the counts
        c->obj_sort_bytes = obj_sort_bytes((long long)N);
        HIPCHK(c, hipMalloc(&c->obj_keys, sizeof(uint64_t) * 2 * N));
        HIPCHK(c, hipMalloc(&c->obj_words, sizeof(int32_t) * (3 * N + 1)));
        HIPCHK(c, hipMalloc(&c->obj_sort_tmp, c->obj_sort_bytes > 0 ? c->obj_sort_bytes : 16));
        c->obj_bytes += (int64_t)(sizeof(uint64_t) * 2 * N + sizeof(int32_t) * (3 * N + 1) + c->obj_sort_bytes);
    }
    if (lists) {  // (the sort's workspace is asked for per size; one sized for the capacity normally holds every batch)
        const size_t need = obj_sort_bytes((long long)c->A.total_pts);
        if (need > c->obj_sort_bytes) {
            HIPCHK(c, hipStreamSynchronize(c->obj_stream ? c->obj_stream : st));
            hipFree(c->obj_sort_tmp);
            c->obj_sort_tmp = nullptr;
            HIPCHK(c, hipMalloc(&c->obj_sort_tmp, need));
            c->obj_bytes += (int64_t)(need - c->obj_sort_bytes);
            c->obj_sort_bytes = need;
        }
    }
    ObjectJob J;
    J.use_track = use_track;
    J.cls = c->rg_done ? c->rg.cls : c->A.pt_type;  // (without the stage: pt_type, whose `other` is tree)
    J.out = (scvod_object*)d_objects;
    J.cap_obj = (long long)cap_objects;
    J.obj_off = d_obj_offsets;
    J.member_src = d_member_src;
    J.cap_mem = (long long)cap_members;
    J.point_object = d_point_object;
    J.tile_cnt = c->obj_tiles;
    J.scan_cnt = c->obj_scan_cnt;
    J.stats = c->obj_stats;
    J.key_in = lists ? c->obj_keys : nullptr;
    J.key_out = lists ? c->obj_keys + N : nullptr;
    J.root_obj = lists ? c->obj_words : nullptr;
    J.nvox = lists ? c->obj_words + N : nullptr;
    J.begin = lists ? c->obj_words + 2 * N : nullptr;
    J.tiles_per_scan = tps;
    if (d_point_object && c->A.total_pts > 0) HIPCHK(c, hipMemsetAsync(d_point_object, 0xff, sizeof(int32_t) * (size_t)c->A.total_pts, st));
    HIPCHK(c, launch_objects(c->A, J, c->obj_sort_tmp, c->obj_sort_bytes, st));
    HIPCHK(c, hipGetLastError());
    c->obj_stream = st;
    c->obj_ran = true;
    if (lists) {  // (a count-only call leaves the lists of an earlier call as they are)
        c->obj_lists_serial = c->cluster_serial;
        c->obj_lists_types_serial = c->types_serial;
        c->obj_lists_track = use_track;
    }
    return SCVOD_OK;
}

int scvod_batch_objects_stats(scvod_ctx* c, int64_t* h_out4) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out4) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->obj_ran) return fail(c, SCVOD_ERR_STATE, "no scvod_batch_objects on this ctx yet");
    HIPCHK(c, hipSetDevice(c->device));
    long long h[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->obj_stats, sizeof(h), hipMemcpyDeviceToHost, c->obj_stream));
    HIPCHK(c, hipStreamSynchronize(c->obj_stream));
    for (int k = 0; k < 4; ++k) h_out4[k] = (int64_t)h[k];
    if (h[3]) return fail(c, SCVOD_ERR_CAPACITY, "the last object table holds %lld objects and %lld member points: a buffer was too small", h[1], h[2]);
    return SCVOD_OK;
}

int64_t scvod_batch_objects_scratch_bytes(scvod_ctx* c) { return c ? c->obj_bytes : 0; }

// ---- the eigenvalue descriptor of the table's objects (k_obj_shape, scvod_objects.hip) ----
void scvod_feature_params_default(scvod_feature_params* p) {
    if (!p) return;
    p->kOneThird = 0.333;  // feature/k*_ (utility.h:318-325)
    p->kLinearityMax = 740.0;
    p->kPlanarityMax = 959.0;
    p->kScatteringMax = 1248.0;
    p->kOmnivarianceMax = 0.278636;
    p->kAnisotropyMax = 1248.0;
    p->kEigenEntropyMax = 0.956129;
    p->kChangeOfCurvatureMax = 0.99702;
}

int scvod_set_object_features(scvod_ctx* c, const scvod_feature_params* p) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!p) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    const double v[8] = {p->kOneThird, p->kLinearityMax, p->kPlanarityMax, p->kScatteringMax, p->kOmnivarianceMax, p->kAnisotropyMax,
                         p->kEigenEntropyMax, p->kChangeOfCurvatureMax};
    if (!finite_d(v[0])) return fail(c, SCVOD_ERR_INVALID, "object features: kOneThird is not finite");
    for (int k = 1; k < 8; ++k)
        if (!(v[k] > 0.0) || !finite_d(v[k])) return fail(c, SCVOD_ERR_INVALID, "object features: every k*Max must be a positive finite number");
    c->feat = FeatureParams{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
    return SCVOD_OK;
}

int scvod_batch_object_shapes(scvod_ctx* c, void* d_shapes, int64_t cap_shapes, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!d_shapes || cap_shapes < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->obj_lists_serial) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_shapes needs a scvod_batch_objects that asked for records or members");
    if (int rc = export_check(c, c->obj_lists_track, "scvod_batch_object_shapes")) return rc;
    if (c->obj_lists_serial != c->cluster_serial)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_shapes: the last object table belongs to an earlier clustering: call scvod_batch_objects again");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    if (!c->shape_stats) {  // first call of this ctx
        HIPCHK(c, hipMalloc(&c->shape_stats, sizeof(long long) * 4));
        c->obj_bytes += (int64_t)(sizeof(long long) * 4);
    }
    const size_t N = (size_t)(c->cap_pts > 0 ? c->cap_pts : 1);
    ShapeJob J;
    J.tab_stats = c->obj_stats;  // what the table left in the scratch; none of its caller's buffers
    J.key_out = c->obj_keys + N;
    J.begin = c->obj_words + 2 * N;
    J.out = (ObjShape*)d_shapes;
    J.cap = (long long)cap_shapes;
    J.stats = c->shape_stats;
    J.K = c->feat;
    launch_object_shapes(c->A, J, st);
    HIPCHK(c, hipGetLastError());
    c->shape_stream = st;
    c->shape_ran = true;
    return SCVOD_OK;
}

int scvod_batch_object_shapes_stats(scvod_ctx* c, int64_t* h_out4) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out4) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->shape_ran) return fail(c, SCVOD_ERR_STATE, "no scvod_batch_object_shapes on this ctx yet");
    HIPCHK(c, hipSetDevice(c->device));
    long long h[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->shape_stats, sizeof(h), hipMemcpyDeviceToHost, c->shape_stream));
    HIPCHK(c, hipStreamSynchronize(c->shape_stream));
    for (int k = 0; k < 4; ++k) h_out4[k] = (int64_t)h[k];
    if (h[3]) return fail(c, SCVOD_ERR_CAPACITY, "the table holds %lld objects, the shape buffer %lld", h[1], h[0]);
    return SCVOD_OK;
}

// the 11-value row of getDescriptorByEigenValue (ssc.cpp:686-751) from a record of the table and, optionally, its shape
void scvod_feature_row(const scvod_object* o, const scvod_object_shape* shape, double* out11) {
    if (!o || !out11) return;
    for (int k = 0; k < 6; ++k) out11[k] = shape ? shape->feat[k] : 1.0;
    out11[6] = (double)o->box_max[2];
    out11[7] = (double)(o->box_max[0] - o->box_min[0]) * (double)(o->box_max[1] - o->box_min[1]);  // diff_x * diff_y: float differences, double product
    out11[8] = (double)o->angle_diff;
    out11[9] = (double)o->box_min[2];
    out11[10] = (double)o->cls;
}

// SSC::compareFeature (ssc.cpp:897-911), literally: a float accumulator that takes ten double products
float scvod_compare_feature(const double* a, const double* b) {
    if (!a || !b) return u2f(0x7fc00000u);
    const double w[10] = {0.5, 0.5, 0.2, 0.2, 0.2, 0.2, 0.2, 0.6, 0.2, 0.0};
    float diff = 0.f;
    for (int k = 0; k < 10; ++k) diff = (float)((double)diff + fabs_d(a[k] - b[k]) * w[k]);
    return diff;
}

// Streaming ingest of a sequence that lives in HOST memory (the reference reads one .bin per scan from disk,
// SSC::getCloud ssc.cpp:1040-1125): chunks of scans are copied host -> device on a copy stream into one of two buffers
// while the previous chunk is processed on the compute stream; `fn` is called once per chunk, after its
// scvod_batch_process launches are enqueued, to enqueue the consumers of that chunk's results (clustering, tracking, map
// accumulation ...) on the same stream -- the arena holds one chunk at a time.
int scvod_sequence_ingest(scvod_ctx* c, const float* h_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, int32_t chunk_scans,
                          int32_t flags, scvod_chunk_fn fn, void* user) {
    if (!c || !h_xyzi || !h_scan_offsets || n_scans <= 0 || chunk_scans <= 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (chunk_scans > c->cap_scans) return fail(c, SCVOD_ERR_CAPACITY, "chunk of %d scans > capacity %d", chunk_scans, c->cap_scans);
    const int n_chunks = (n_scans + chunk_scans - 1) / chunk_scans;
    int64_t max_chunk_pts = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const int s0 = k * chunk_scans, s1 = s0 + chunk_scans < n_scans ? s0 + chunk_scans : n_scans;
        const int64_t p = (int64_t)h_scan_offsets[s1] - h_scan_offsets[s0];
        if (p < 0) return fail(c, SCVOD_ERR_INVALID, "scan_offsets not monotone");
        if (p > max_chunk_pts) max_chunk_pts = p;
    }
    if (max_chunk_pts > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "chunk of %lld points > capacity %lld", (long long)max_chunk_pts, (long long)c->cap_pts);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->copy_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
        if (!c->ingest_copied[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ingest_copied[k], hipEventDisableTiming));
        if (!c->ingest_done[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ingest_done[k], hipEventDisableTiming));
    }
    if ((size_t)max_chunk_pts > c->ingest_cap) {
        HIPCHK(c, hipDeviceSynchronize());
        for (int k = 0; k < 2; ++k) {
            if (c->ingest_buf[k]) hipFree(c->ingest_buf[k]);
            c->ingest_buf[k] = nullptr;
        }
        c->ingest_cap = 0;
        for (int k = 0; k < 2; ++k) HIPCHK(c, hipMalloc(&c->ingest_buf[k], 16 * (size_t)max_chunk_pts));
        c->ingest_cap = (size_t)max_chunk_pts;
    }
    const size_t off_need = (size_t)n_scans + (size_t)n_chunks + 8;
    if (off_need > c->ingest_off_cap) {
        HIPCHK(c, hipDeviceSynchronize());
        if (c->ingest_off) hipHostFree(c->ingest_off);
        c->ingest_off = nullptr;
        c->ingest_off_cap = 0;
        HIPCHK(c, hipHostMalloc((void**)&c->ingest_off, sizeof(int32_t) * off_need, hipHostMallocDefault));
        c->ingest_off_cap = off_need;
    }
    const size_t bytes_all = 16 * (size_t)(h_scan_offsets[n_scans] - h_scan_offsets[0]);
    bool registered = false;
    if ((flags & SCVOD_INGEST_REGISTER) && bytes_all) {  // pin the caller's buffer for the duration of the call
        if (hipHostRegister((void*)(h_xyzi + 4 * (size_t)h_scan_offsets[0]), bytes_all, hipHostRegisterDefault) == hipSuccess)
            registered = true;
        else
            (void)hipGetLastError();  // already pinned or not registrable: the copies still work (staged)
    }
    hipStream_t st = c->stream;
    int rc = SCVOD_OK;
    int32_t* po = c->ingest_off;
    for (int k = 0; k < n_chunks && rc == SCVOD_OK; ++k) {
        const int b = k & 1;
        const int s0 = k * chunk_scans, s1 = s0 + chunk_scans < n_scans ? s0 + chunk_scans : n_scans;
        const int ns = s1 - s0;
        for (int j = 0; j <= ns; ++j) po[j] = h_scan_offsets[s0 + j] - h_scan_offsets[s0];
        const size_t npts = (size_t)po[ns];
        // the buffer is free once the consumers of the chunk two steps back are done
        if (k >= 2 && hipStreamWaitEvent(c->copy_stream, c->ingest_done[b], 0) != hipSuccess) rc = fail(c, SCVOD_ERR_HIP, "hipStreamWaitEvent");
        if (rc == SCVOD_OK && npts &&
            hipMemcpyAsync(c->ingest_buf[b], h_xyzi + 4 * (size_t)h_scan_offsets[s0], 16 * npts, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess)
            rc = fail(c, SCVOD_ERR_HIP, "hipMemcpyAsync (ingest)");
        if (rc == SCVOD_OK && (hipEventRecord(c->ingest_copied[b], c->copy_stream) != hipSuccess ||
                               hipStreamWaitEvent(st, c->ingest_copied[b], 0) != hipSuccess))
            rc = fail(c, SCVOD_ERR_HIP, "ingest event");
        if (rc == SCVOD_OK) rc = run_batch(c, c->ingest_buf[b], po, ns, st, 1, 1, 1, 0, true, true);
        if (rc == SCVOD_OK && fn) {
            const int frc = fn(user, c, s0, ns, (void*)st);
            if (frc != SCVOD_OK) rc = fail(c, frc, "chunk callback returned %d", frc);
        }
        if (rc == SCVOD_OK && hipEventRecord(c->ingest_done[b], st) != hipSuccess) rc = fail(c, SCVOD_ERR_HIP, "hipEventRecord");
        po += ns + 1;
    }
    hipError_t e1 = hipStreamSynchronize(c->copy_stream), e2 = hipStreamSynchronize(st);
    if (registered) hipHostUnregister((void*)(h_xyzi + 4 * (size_t)h_scan_offsets[0]));
    if (rc == SCVOD_OK && (e1 != hipSuccess || e2 != hipSuccess)) rc = fail(c, SCVOD_ERR_HIP, "ingest: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    return rc;
}

int scvod_set_timing(scvod_ctx* c, int32_t enabled) {
    if (!c) return SCVOD_ERR_INVALID;
    c->timing = enabled != 0;
    return SCVOD_OK;
}

int scvod_batch_timings(scvod_ctx* c, const char** names, float* ms, int32_t cap) {
    if (!c) return SCVOD_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess) return SCVOD_ERR_HIP;
    if (c->last_stream) hipStreamSynchronize(c->last_stream);
    int n = 0;
    for (size_t i = 0; i < c->tim_used && n < cap; ++i, ++n) {
        float t = 0.f;
        hipEventElapsedTime(&t, c->tim[i].e0, c->tim[i].e1);
        if (names) names[n] = c->tim[i].name;
        if (ms) ms[n] = t;
    }
    return n;
}

int scvod_batch_voxelgrid(scvod_ctx* c, const void* d_xyzi, const uint32_t* d_labels, const int32_t* h_scan_offsets,
                          int32_t n_scans, const float leaf[3], float max_intensity, void* d_out_xyzi, int64_t out_capacity,
                          int32_t* h_out_offsets, void* stream) {
    return run_voxelgrid(c, d_xyzi, d_labels, h_scan_offsets, n_scans, leaf, max_intensity, d_out_xyzi, out_capacity,
                         h_out_offsets, (hipStream_t)stream);
}

int scvod_voxelgrid(scvod_ctx* c, const float* h_xyzi, const uint32_t* h_labels, int32_t n, const float leaf[3],
                    float max_intensity, float* h_out_xyzi, int32_t out_capacity, int32_t* n_out) {
    if (!c || !n_out || n < 0 || (n > 0 && (!h_xyzi || !h_out_xyzi))) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    *n_out = 0;
    if (n == 0) return SCVOD_OK;
    if (n > c->cap_pts) return fail(c, SCVOD_ERR_CAPACITY, "%d points > capacity %lld", n, (long long)c->cap_pts);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc_side = ensure_side(c, kSideIn | (h_labels ? kSideLabels : 0))) return rc_side;
    HIPCHK(c, hipMemcpyAsync(c->d_in, h_xyzi, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (h_labels) HIPCHK(c, hipMemcpyAsync(c->d_labels, h_labels, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    float4* d_out = (float4*)c->A.cl_bbox;  // device-side output staging: 24 bytes per point, idle outside cluster typing
    int32_t off[2] = {0, n}, out_off[2] = {0, 0};
    int rc = run_voxelgrid(c, c->d_in, h_labels ? c->d_labels : nullptr, off, 1, leaf, max_intensity, d_out, n, out_off, c->stream);
    if (rc) return rc;
    *n_out = out_off[1];
    if (out_off[1] > out_capacity) return fail(c, SCVOD_ERR_CAPACITY, "output buffer too small (%d < %d)", out_capacity, out_off[1]);
    if (out_off[1]) HIPCHK(c, hipMemcpy(h_out_xyzi, d_out, sizeof(float) * 4 * (size_t)out_off[1], hipMemcpyDeviceToHost));
    return SCVOD_OK;
}

// grow-only device scratch owned by the ctx (no allocation on the steady-state path, nothing to leak on an error return): at least
// `bytes` in s.  A block that grows is freed first, after the calls in flight that may still read it: the last one on s, and on
// also_wait where a second kind of call works in the same block
static int scratch_reserve(scvod_ctx* c, Scratch& s, size_t bytes, const Scratch* also_wait = nullptr) {
    if (bytes <= s.cap) return SCVOD_OK;
    if (s.buf) {
        if (s.ran) HIPCHK(c, hipStreamSynchronize(s.stream));
        if (also_wait && also_wait->ran) HIPCHK(c, hipStreamSynchronize(also_wait->stream));
        hipFree(s.buf);
        s.buf = nullptr;
        s.cap = 0;
    }
    const size_t grown = bytes + bytes / 4;
    HIPCHK(c, hipMalloc(&s.buf, grown));
    s.cap = grown;
    return SCVOD_OK;
}

// the counter words of a stage, allocated and cleared by its first call.  An allocation of their own: a grown scratch block must not
// take an unread result with it
static int counter_block(scvod_ctx* c, unsigned long long** words, int n) {
    if (*words) return SCVOD_OK;
    HIPCHK(c, hipMalloc(words, sizeof(unsigned long long) * n));
    HIPCHK(c, hipMemset(*words, 0, sizeof(unsigned long long) * n));
    return SCVOD_OK;
}

// n (<= 24) counter words as they are once the work on `stream` is done
static int read_counters(scvod_ctx* c, const unsigned long long* d_words, int n, hipStream_t stream, int64_t* out) {
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long h[24] = {0};
    HIPCHK(c, hipMemcpyAsync(h, d_words, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    for (int k = 0; k < n; ++k) out[k] = (int64_t)h[k];
    return SCVOD_OK;
}

static int nn_run(scvod_ctx* c, const float* d_map, int32_t n_map, const float* d_q, int32_t n_query, float radius,
                  int32_t* d_idx, float* d_sq, uint8_t* d_w, const float origin[3], int bounded, hipStream_t st) {
    // grid: cell edge >= radius; the origin only shifts the hash.  The radius search answers from the 27 cells alone, which hold every
    // point closer than 0.99 cell edges (launch_nn's h2) and no promise beyond: its cell is widened until radius^2 <= h2
    float cell = radius > 0.2f ? radius : 0.2f;
    if (bounded && radius * radius > (0.99f * cell) * (0.99f * cell)) cell = radius / 0.98f;
    const int32_t buckets = grid_buckets(n_map);
    const size_t nm = n_map ? n_map : 1, nq = n_query ? n_query : 1;
    const size_t work_ints = 3 * (size_t)buckets + nm + nq + 8 + (size_t)buckets / 1024 + 1;
    if (int rc = scratch_reserve(c, c->nn[5], work_ints * sizeof(int))) return rc;
    launch_nn(d_map, n_map, d_q, n_query, radius, d_idx, d_sq, d_w, origin, cell, buckets, (int*)c->nn[5].buf, bounded, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

static int nn_search_host(scvod_ctx* c, const float* h_map_xyz, int32_t n_map, const float* h_query_xyz, int32_t n_query, float radius,
                          int32_t* h_nn_idx, float* h_nn_sqdist, uint8_t* h_within, int bounded) {
    if (!c || n_map < 0 || n_query < 0 || (n_map > 0 && !h_map_xyz) || (n_query > 0 && !h_query_xyz))
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nm = n_map ? n_map : 1, nq = n_query ? n_query : 1;
    float origin[3] = {0.f, 0.f, 0.f};  // min corner of the map (keeps the cell coordinates small)
    for (int i = 0; i < n_map; ++i)
        for (int k = 0; k < 3; ++k)
            if (i == 0 || h_map_xyz[3 * (size_t)i + k] < origin[k]) origin[k] = h_map_xyz[3 * (size_t)i + k];
    const size_t bytes[5] = {nm * 12, nq * 12, nq * 4, nq * 4, nq};
    int rc;
    for (int k = 0; k < 5; ++k)
        if ((rc = scratch_reserve(c, c->nn[k], bytes[k]))) return rc;
    void *d_map = c->nn[0].buf, *d_q = c->nn[1].buf, *d_sq = c->nn[2].buf, *d_idx = c->nn[3].buf, *d_w = c->nn[4].buf;
    hipStream_t st = c->stream;
    if (n_map) HIPCHK(c, hipMemcpyAsync(d_map, h_map_xyz, (size_t)n_map * 12, hipMemcpyHostToDevice, st));
    if (n_query) HIPCHK(c, hipMemcpyAsync(d_q, h_query_xyz, (size_t)n_query * 12, hipMemcpyHostToDevice, st));
    if ((rc = nn_run(c, (const float*)d_map, n_map, (const float*)d_q, n_query, radius, (int32_t*)d_idx, (float*)d_sq, (uint8_t*)d_w,
                     origin, bounded, st)))
        return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    if (n_query) {
        if (h_nn_idx) HIPCHK(c, hipMemcpy(h_nn_idx, d_idx, (size_t)n_query * 4, hipMemcpyDeviceToHost));
        if (h_nn_sqdist) HIPCHK(c, hipMemcpy(h_nn_sqdist, d_sq, (size_t)n_query * 4, hipMemcpyDeviceToHost));
        if (h_within) HIPCHK(c, hipMemcpy(h_within, d_w, (size_t)n_query, hipMemcpyDeviceToHost));
        // (an empty map: k_nn_brute leaves distance 0 beside index -1; the radius search promises +inf)
        if (bounded && n_map == 0 && h_nn_sqdist) std::fill(h_nn_sqdist, h_nn_sqdist + n_query, std::numeric_limits<float>::infinity());
    }
    return SCVOD_OK;
}

int scvod_nn_search(scvod_ctx* c, const float* h_map_xyz, int32_t n_map, const float* h_query_xyz, int32_t n_query,
                    float radius, int32_t* h_nn_idx, float* h_nn_sqdist, uint8_t* h_within) {
    return nn_search_host(c, h_map_xyz, n_map, h_query_xyz, n_query, radius, h_nn_idx, h_nn_sqdist, h_within, 0);
}
int scvod_nn_radius_search(scvod_ctx* c, const float* h_map_xyz, int32_t n_map, const float* h_query_xyz, int32_t n_query,
                           float radius, int32_t* h_nn_idx, float* h_nn_sqdist) {
    if (!(radius > 0.f)) return fail(c, SCVOD_ERR_INVALID, "radius must be positive");
    std::vector<uint8_t> w(n_query > 0 ? n_query : 1);
    return nn_search_host(c, h_map_xyz, n_map, h_query_xyz, n_query, radius, h_nn_idx, h_nn_sqdist, w.data(), 1);
}

int scvod_nn_search_device(scvod_ctx* c, const float* d_map_xyz, int32_t n_map, const float* d_query_xyz, int32_t n_query,
                           float radius, int32_t* d_nn_idx, float* d_nn_sqdist, uint8_t* d_within, void* stream) {
    if (!c || n_map < 0 || n_query < 0 || (n_map > 0 && !d_map_xyz) || (n_query > 0 && (!d_query_xyz || !d_nn_idx || !d_nn_sqdist || !d_within)))
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const float origin[3] = {0.f, 0.f, 0.f};
    return nn_run(c, d_map_xyz, n_map, d_query_xyz, n_query, radius, d_nn_idx, d_nn_sqdist, d_within, origin, 0,
                  stream ? (hipStream_t)stream : c->stream);
}

// ---- evaluation against labelled truth, on the device (scvod_eval.hip) ----
void scvod_eval_params_default(scvod_eval_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->voxelsize = 0.2;
    p->n_dynamic_classes = 8;
    for (int k = 0; k < 8; ++k) p->dynamic_classes[k] = (uint16_t)(252 + k);  // analysis.py:6
}

void scvod_eval_finish(const int64_t counts[7], scvod_eval_result* out) {
    if (!counts || !out) return;
    out->num_gt_static = counts[0];
    out->num_gt_dynamic = counts[1];
    out->num_est_static = counts[2];
    out->num_est_dynamic = counts[3];
    out->num_preserved = counts[4];
    out->num_static_preserved = counts[5];
    out->num_dynamic_preserved = counts[6];
    const double nan = std::nan("");
    // analysis.py:186-190 / metric.py:28-30, operation by operation (the library is built without contraction)
    const double pr = counts[0] ? 100.0 * (double)counts[5] / (double)counts[0] : nan;
    const double rr = counts[1] ? 100.0 * (double)(counts[1] - counts[6]) / (double)counts[1] : nan;
    double f1 = nan;  // (a rate without a denominator: analysis.py would raise)
    if (counts[0] && counts[1]) f1 = pr + rr > 0 ? 2.0 * (pr / 100.0) * (rr / 100.0) / ((pr / 100.0) + (rr / 100.0)) : 0.0;
    out->PR = pr;
    out->RR = rr;
    out->F1 = f1;
}

// the parameters of a call (NULL: the defaults) as the kernels take them; argument errors only
static int ev_params(scvod_ctx* c, const scvod_eval_params* params, EvClasses* K, double* voxelsize) {
    scvod_eval_params p;
    if (params)
        p = *params;
    else
        scvod_eval_params_default(&p);
    if (p.n_dynamic_classes < 0 || p.n_dynamic_classes > 16) return fail(c, SCVOD_ERR_INVALID, "%d dynamic classes (0..16)", p.n_dynamic_classes);
    if (!(p.voxelsize > 0.0) || !std::isfinite(p.voxelsize)) return fail(c, SCVOD_ERR_INVALID, "voxelsize must be positive and finite");
    memset(K, 0, sizeof(*K));
    K->n = p.n_dynamic_classes;
    for (int k = 0; k < K->n; ++k) K->c[k] = p.dynamic_classes[k];
    *voxelsize = p.voxelsize;
    return SCVOD_OK;
}

// the evaluation's scratch block of at least `bytes` (growing waits for the evaluations and the map classifications in flight)
static int ev_reserve(scvod_ctx* c, size_t bytes) {
    if (int rc = counter_block(c, &c->ev_counters, 16)) return rc;
    return scratch_reserve(c, c->ev, bytes, &c->ev_cls);
}

static float ev_cell(double radius) {  // the cell edge is at least the radius, so the 27-cell probe of scvod_grid.h decides it
    const float r = (float)radius;
    return r > 0.2f ? r : 0.2f;
}

// the batch as a cloud against itself, what scvod_batch_evaluate and scvod_batch_score_classes (`who`) share: the world position of
// every input point of the batch, its keep byte (scvod_batch_export_points' rule for `flags`, and the bits of keep_extra) and its
// SCVOD_PT_* byte (class_byte: the class byte where the region growing ran), in the stage's scratch block:
//     world xyz | keep byte | label or class byte | pose matrices | the stage's work area of work_bytes(buckets, n)
// The checks come in the order arguments, flags, parameters (parse_params), state of the batch, device.
struct BatchCloud {
    float* world;
    uint8_t *keep, *byte;
    int* work;
    int32_t n, buckets;
    hipStream_t st;
};
static int batch_cloud(scvod_ctx* c, const char* who, const uint32_t* d_gt_label, const float* h_poses, int32_t flags,
                       const std::function<int()>& parse_params, uint32_t keep_extra, bool class_byte, Scratch& block, int (*reserve)(scvod_ctx*, size_t),
                       size_t (*work_bytes)(int32_t buckets, int32_t n), void* stream, BatchCloud* out) {
    if (!d_gt_label || !h_poses) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (flags & ~(SCVOD_MAP_NO_GROUND | SCVOD_MAP_NO_REJECTED | SCVOD_MAP_IGNORE_DYNAMIC))
        return fail(c, SCVOD_ERR_INVALID, "%s takes SCVOD_MAP_NO_GROUND, SCVOD_MAP_NO_REJECTED and SCVOD_MAP_IGNORE_DYNAMIC only (flags %d)", who, flags);
    if (int rc = parse_params()) return rc;
    const int use_dyn = (flags & SCVOD_MAP_IGNORE_DYNAMIC) ? 0 : 1;
    if (int rc = export_check(c, use_dyn, who)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    const int B = c->A.n_scans;
    const int32_t N = (int32_t)c->A.total_pts;
    const int32_t buckets = grid_buckets(N);
    const size_t n1 = (size_t)(N > 0 ? N : 1);
    const size_t off_keep = align_up(12 * n1, 256), off_byte = off_keep + align_up(n1, 256), off_pose = off_byte + align_up(n1, 256),
                 off_work = off_pose + align_up(sizeof(float) * 12 * (size_t)(B > 0 ? B : 1), 256);
    if (int rc = reserve(c, off_work + work_bytes(buckets, N))) return rc;
    unsigned char* base = (unsigned char*)block.buf;
    float* world = (float*)base;
    uint8_t* keep = base + off_keep;
    uint8_t* byte = base + off_byte;
    float* pose = (float*)(base + off_pose);
    if (B > 0) {  // pcl::getTransformation per scan, staged before the call returns: h_poses is the caller's again at once
        std::vector<float> T((size_t)12 * B);
        for (int s = 0; s < B; ++s) scvod_pose_matrix(h_poses + 6 * s, T.data() + 12 * s);
        if (int rc = staged_upload(c, T.data(), sizeof(float) * T.size(), pose, st)) return rc;
    }
    uint32_t keep_mask = (1u << SCVOD_PT_UNCLUSTERED) | (1u << SCVOD_PT_STATIC_OTHER) | (1u << SCVOD_PT_STATIC_CAR) | keep_extra;
    if (!(flags & SCVOD_MAP_NO_GROUND)) keep_mask |= 1u << SCVOD_PT_GROUND;
    if (!(flags & SCVOD_MAP_NO_REJECTED)) keep_mask |= 1u << SCVOD_PT_REJECTED;
    if (!use_dyn) keep_mask |= 1u << SCVOD_PT_DYNAMIC;
    if (N > 0) {
        HIPCHK(c, hipMemsetAsync(byte, SCVOD_PT_DROPPED, (size_t)N, st));
        if (int rc = ensure_lists(c, st)) return rc;
        if (class_byte && c->rg_done)
            launch_point_classes(c->A, c->rg.cls, byte, use_dyn, st);
        else
            launch_point_labels(c->A, byte, use_dyn, st);
        launch_eval_world(c->A, byte, keep_mask, pose, world, keep, st);  // (k_ev_world: the export's expression and keep rule)
    }
    *out = BatchCloud{world, keep, byte, (int*)(base + off_work), N, buckets, st};
    return SCVOD_OK;
}

int scvod_evaluate_device(scvod_ctx* c, const float* d_gt_xyz, const uint32_t* d_gt_label, int32_t n_gt, const float* d_est_xyz,
                          const uint32_t* d_est_label, int32_t n_est, const scvod_eval_params* params, uint8_t* d_point_result, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_gt < 0 || n_est < 0 || (n_gt > 0 && (!d_gt_xyz || !d_gt_label)) || (n_est > 0 && (!d_est_xyz || !d_est_label)))
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    EvClasses K;
    double vs;
    if (int rc = ev_params(c, params, &K, &vs)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const int32_t buckets = grid_buckets(n_est);
    if (int rc = ev_reserve(c, sizeof(int) * grid_work_ints(buckets, n_est))) return rc;
    launch_eval(d_gt_xyz, d_gt_label, n_gt, d_est_xyz, d_est_label, nullptr, n_est, vs * std::sqrt(3.0) / 2, K, ev_cell(vs), buckets,
                (int*)c->ev.buf, c->ev_counters, d_point_result, st);
    HIPCHK(c, hipGetLastError());
    c->ev.stream = st;
    c->ev.ran = true;
    return SCVOD_OK;
}

int scvod_batch_evaluate(scvod_ctx* c, const uint32_t* d_gt_label, const float* h_poses, int32_t flags, const scvod_eval_params* params,
                         uint8_t* d_point_result, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    EvClasses K;
    double vs;
    BatchCloud W;
    if (int rc = batch_cloud(c, "scvod_batch_evaluate", d_gt_label, h_poses, flags, [&] { return ev_params(c, params, &K, &vs); }, 0u, false, c->ev,
                             ev_reserve, [](int32_t buckets, int32_t n) { return sizeof(int) * grid_work_ints(buckets, n); }, stream, &W))
        return rc;
    launch_eval(W.world, d_gt_label, W.n, W.world, d_gt_label, W.keep, W.n, vs * std::sqrt(3.0) / 2, K, ev_cell(vs), W.buckets, W.work,
                c->ev_counters, d_point_result, W.st);
    HIPCHK(c, hipGetLastError());
    c->ev.stream = W.st;
    c->ev.ran = true;
    return SCVOD_OK;
}

int scvod_evaluate_stats(scvod_ctx* c, scvod_eval_result* out) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!out) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->ev.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_evaluate_device or scvod_batch_evaluate on this ctx yet");
    int64_t counts[7];
    if (int rc = read_counters(c, c->ev_counters, 7, c->ev.stream, counts)) return rc;
    scvod_eval_finish(counts, out);
    return SCVOD_OK;
}

int64_t scvod_evaluate_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->ev.cap + (c->ev_counters ? (int64_t)sizeof(unsigned long long) * 16 : 0) : 0;
}

int scvod_classify_map_device(scvod_ctx* c, const float* d_orig_xyz, const uint8_t* d_pred_static, int32_t n, const float* d_static_xyz,
                              int32_t n_static, const float* d_dynamic_xyz, int32_t n_dynamic, float r15, float r10, uint8_t* d_class, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n < 0 || n_static < 0 || n_dynamic < 0 || (n > 0 && (!d_orig_xyz || !d_pred_static)) || (n_static > 0 && !d_static_xyz) ||
        (n_dynamic > 0 && !d_dynamic_xyz))
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    const float cell = 0.2f;
    if (!(r15 > 0.f) || !(r10 > 0.f) || r15 > 0.99f * cell || r10 > 0.99f * cell)
        return fail(c, SCVOD_ERR_INVALID, "radii %g / %g: positive and at most 0.99 cell edges of 0.2", (double)r15, (double)r10);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const int32_t bs = grid_buckets(n_static), bd = grid_buckets(n_dynamic);
    const size_t off_d = align_up(sizeof(int) * grid_work_ints(bs, n_static), 256);
    if (int rc = ev_reserve(c, off_d + sizeof(int) * grid_work_ints(bd, n_dynamic))) return rc;
    unsigned char* base = (unsigned char*)c->ev.buf;
    launch_classify(d_orig_xyz, d_pred_static, n, d_static_xyz, n_static, d_dynamic_xyz, n_dynamic, r15, r10, cell, bs, (int*)base, bd,
                    (int*)(base + off_d), c->ev_counters + 8, d_class, st);
    HIPCHK(c, hipGetLastError());
    c->ev_cls.stream = st;
    c->ev_cls.ran = true;
    return SCVOD_OK;
}

int scvod_classify_map_stats(scvod_ctx* c, int64_t* h_out5) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out5) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->ev_cls.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_classify_map_device on this ctx yet");
    return read_counters(c, c->ev_counters + 8, 5, c->ev_cls.stream, h_out5);
}

// ---- class scores against labelled truth (scvod_classes.hip) ----
void scvod_class_params_default(scvod_class_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_dist = 0.75f;
    p->cell = 0.25f;
    const uint16_t g[6] = {40, 44, 48, 49, 71, 72}, b[4] = {50, 51, 52, 60}, t[3] = {70, 80, 81};  // plotObject.cpp:3-5
    p->n_ground = 6;
    p->n_building = 4;
    p->n_tree = 3;
    for (int k = 0; k < 6; ++k) p->ground[k] = g[k];
    for (int k = 0; k < 4; ++k) p->building[k] = b[k];
    for (int k = 0; k < 3; ++k) p->tree[k] = t[k];
}

void scvod_class_finish(const int64_t conf_and_far[21], scvod_class_result* out) {
    if (!conf_and_far || !out) return;
    for (int t = 0; t < 4; ++t) {
        int64_t num = 0;
        for (int e = 0; e < 5; ++e) num += (out->conf[t][e] = conf_and_far[t * 5 + e]);
        out->num[t] = num;
    }
    out->pd_far = conf_and_far[20];
    out->P[0] = out->conf[0][1];
    out->P[1] = out->conf[1][2] + out->conf[1][3];
    out->P[2] = out->conf[2][2] + out->conf[2][3];
    out->P[3] = out->conf[3][0] + out->conf[3][4] + out->pd_far;
    for (int t = 0; t < 4; ++t) {  // plotObject.cpp:143-146: (float)P / num, 0 / 0 prints nan
        out->rate_P[t] = (float)out->P[t] / (float)out->num[t];
        out->rate_N[t] = (float)(out->num[t] - out->P[t]) / (float)out->num[t];
    }
}

// the parameters of a call (NULL: the defaults) as the kernels take them; argument errors only
static int cs_params(scvod_ctx* c, const scvod_class_params* params, CsLists* L, float* cell, float* max_dist, int32_t* rings) {
    scvod_class_params p;
    if (params)
        p = *params;
    else
        scvod_class_params_default(&p);
    if (p.n_ground < 0 || p.n_ground > 8 || p.n_building < 0 || p.n_building > 8 || p.n_tree < 0 || p.n_tree > 8)
        return fail(c, SCVOD_ERR_INVALID, "class lists of %d / %d / %d labels (0..8 each)", p.n_ground, p.n_building, p.n_tree);
    if (!(p.cell > 0.f) || !std::isfinite(p.cell) || !(p.max_dist > 0.f) || !std::isfinite(p.max_dist))
        return fail(c, SCVOD_ERR_INVALID, "cell and max_dist must be positive and finite");
    if (!(p.max_dist * p.max_dist > 0.5f) || !std::isfinite(p.max_dist * p.max_dist))
        return fail(c, SCVOD_ERR_INVALID, "max_dist %g: max_dist * max_dist must exceed 0.5 (the pd rule's distance)", (double)p.max_dist);
    const double r = std::ceil((double)p.max_dist / (0.99 * (double)p.cell));
    if (!(r <= 32.0)) return fail(c, SCVOD_ERR_INVALID, "max_dist %g spans more than 32 rings of cells of %g", (double)p.max_dist, (double)p.cell);
    memset(L, 0, sizeof(*L));
    L->n_ground = p.n_ground;
    L->n_building = p.n_building;
    L->n_tree = p.n_tree;
    for (int k = 0; k < 8; ++k) {
        L->ground[k] = p.ground[k];
        L->building[k] = p.building[k];
        L->tree[k] = p.tree[k];
    }
    *cell = p.cell;
    *max_dist = p.max_dist;
    *rings = r < 1.0 ? 1 : (int32_t)r;
    return SCVOD_OK;
}

// the scoring's scratch block of at least `bytes` (growing waits for the scoring in flight)
static int cs_reserve(scvod_ctx* c, size_t bytes) {
    if (int rc = counter_block(c, &c->cs_counters, 24)) return rc;
    return scratch_reserve(c, c->cs, bytes);
}

int scvod_score_classes_device(scvod_ctx* c, const float* d_gt_xyz, const uint32_t* d_gt_label, int32_t n_gt, const float* d_est_xyz,
                               const uint8_t* d_est_class, int32_t n_est, const scvod_class_params* params, uint8_t* d_point_result,
                               void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_gt < 0 || n_est < 0 || (n_gt > 0 && (!d_gt_xyz || !d_gt_label)) || (n_est > 0 && (!d_est_xyz || !d_est_class)))
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    CsLists L;
    float cell, max_dist;
    int32_t rings;
    if (int rc = cs_params(c, params, &L, &cell, &max_dist, &rings)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const int32_t buckets = grid_buckets(n_est);
    if (int rc = cs_reserve(c, cs_work_bytes(buckets, n_est, n_gt))) return rc;
    launch_class_score(d_gt_xyz, d_gt_label, n_gt, d_est_xyz, d_est_class, nullptr, n_est, L, cell, max_dist, rings, buckets, (int*)c->cs.buf,
                       c->cs_counters, d_point_result, st);
    HIPCHK(c, hipGetLastError());
    c->cs.stream = st;
    c->cs.ran = true;
    return SCVOD_OK;
}

int scvod_batch_score_classes(scvod_ctx* c, const uint32_t* d_gt_label, const float* h_poses, int32_t flags, const scvod_class_params* params,
                              uint8_t* d_point_result, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    CsLists L;
    float cell, max_dist;
    int32_t rings;
    BatchCloud W;
    // a building point is kept as the STATIC_OTHER point it is for the export
    if (int rc = batch_cloud(c, "scvod_batch_score_classes", d_gt_label, h_poses, flags, [&] { return cs_params(c, params, &L, &cell, &max_dist, &rings); },
                             1u << SCVOD_PT_STATIC_BUILDING, true, c->cs, cs_reserve, [](int32_t buckets, int32_t n) { return cs_work_bytes(buckets, n, n); },
                             stream, &W))
        return rc;
    launch_class_score(W.world, d_gt_label, W.n, W.world, W.byte, W.keep, W.n, L, cell, max_dist, rings, W.buckets, W.work, c->cs_counters,
                       d_point_result, W.st);
    HIPCHK(c, hipGetLastError());
    c->cs.stream = W.st;
    c->cs.ran = true;
    return SCVOD_OK;
}

int scvod_score_classes_stats(scvod_ctx* c, scvod_class_result* out) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!out) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->cs.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_score_classes_device or scvod_batch_score_classes on this ctx yet");
    int64_t counts[21];
    if (int rc = read_counters(c, c->cs_counters, 21, c->cs.stream, counts)) return rc;
    scvod_class_finish(counts, out);
    return SCVOD_OK;
}

int64_t scvod_score_classes_pass2_queries(scvod_ctx* c) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!c->cs.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_score_classes_device or scvod_batch_score_classes on this ctx yet");
    int64_t n = 0;
    if (int rc = read_counters(c, c->cs_counters + 21, 1, c->cs.stream, &n)) return rc;
    return n;
}

int64_t scvod_score_classes_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->cs.cap + (c->cs_counters ? (int64_t)sizeof(unsigned long long) * 24 : 0) : 0;
}

// ---- object scores: removal per labelled object (scvod_instances.hip) ----
void scvod_instance_params_default(scvod_instance_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    const uint16_t st[8] = {10, 31, 30, 32, 16, 13, 18, 20};  // the static counterparts of 252..259, in that order
    p->n_dynamic_classes = 8;
    p->n_static_classes = 8;
    for (int k = 0; k < 8; ++k) {
        p->dynamic_classes[k] = (uint16_t)(252 + k);
        p->static_classes[k] = st[k];
    }
    p->removed_below = 0.5;
    p->retained_from = 0.5;
    p->min_points = 1;
}

int scvod_instance_finish(const scvod_instance* table, int64_t n, const scvod_instance_params* params, scvod_instance_result* out) {
    if (n < 0 || (n > 0 && !table) || !out) return SCVOD_ERR_INVALID;
    scvod_instance_params p;
    if (params)
        p = *params;
    else
        scvod_instance_params_default(&p);
    if (p.n_dynamic_classes < 0 || p.n_dynamic_classes > 16 || p.n_static_classes < 0 || p.n_static_classes > 16 ||
        !std::isfinite(p.removed_below) || !std::isfinite(p.retained_from))
        return SCVOD_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    for (int64_t i = 0; i < n; ++i) {
        const scvod_instance& r = table[i];
        const uint16_t sem = (uint16_t)(r.label & 0xFFFFu);
        bool dyn = false, stat = false;
        for (int k = 0; k < p.n_dynamic_classes; ++k) dyn |= sem == p.dynamic_classes[k];
        for (int k = 0; k < p.n_static_classes; ++k) stat |= sem == p.static_classes[k];
        if ((r.label >> 16) == 0 || r.n_points < p.min_points || !(dyn || stat)) {
            ++out->skipped;
        } else if (dyn) {
            ++out->hd_gt;
            out->hd_points += r.n_points;
            out->hd_points_preserved += r.n_preserved;
            if ((double)r.n_preserved < p.removed_below * (double)r.n_points) ++out->hd_removed;
        } else {
            ++out->ld_gt;
            out->ld_points += r.n_points;
            out->ld_points_preserved += r.n_preserved;
            if ((double)r.n_preserved >= p.retained_from * (double)r.n_points) ++out->ld_retained;
        }
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();  // scvod_eval_finish's rule for a zero denominator
    out->hd_removed_rate = out->hd_gt ? 100.0 * (double)out->hd_removed / (double)out->hd_gt : nan;
    out->ld_retained_rate = out->ld_gt ? 100.0 * (double)out->ld_retained / (double)out->ld_gt : nan;
    return SCVOD_OK;
}

int scvod_instance_merge(const scvod_instance* a, int64_t na, const scvod_instance* b, int64_t nb, scvod_instance* out, int64_t cap,
                         int64_t* n_out) {
    if (na < 0 || nb < 0 || cap < 0 || (na > 0 && !a) || (nb > 0 && !b) || (cap > 0 && !out) || !n_out) return SCVOD_ERR_INVALID;
    for (int64_t i = 1; i < na; ++i)
        if (!(a[i - 1].label < a[i].label)) return SCVOD_ERR_INVALID;
    for (int64_t i = 1; i < nb; ++i)
        if (!(b[i - 1].label < b[i].label)) return SCVOD_ERR_INVALID;
    int64_t i = 0, j = 0, m = 0;
    while (i < na || j < nb) {
        scvod_instance r;
        if (j >= nb || (i < na && a[i].label < b[j].label)) {
            r = a[i++];
        } else if (i >= na || b[j].label < a[i].label) {
            r = b[j++];
        } else {
            r = a[i++];
            const scvod_instance& o = b[j++];
            r.first_point = o.first_point < r.first_point ? o.first_point : r.first_point;
            r.n_points += o.n_points;
            r.n_inlier += o.n_inlier;
            r.n_preserved += o.n_preserved;
        }
        if (m < cap) out[m] = r;
        ++m;
    }
    *n_out = m;
    return m > cap ? SCVOD_ERR_CAPACITY : SCVOD_OK;
}

int scvod_score_instances_device(scvod_ctx* c, const uint32_t* d_key, const uint8_t* d_point_result, int64_t n, scvod_instance* d_instances,
                                 int32_t cap_instances, int64_t* d_n, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n < 0 || n > (int64_t)INT32_MAX || (n > 0 && (!d_key || !d_point_result)) || !d_n)
        return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (cap_instances < 1 || cap_instances > (1 << 22))
        return fail(c, SCVOD_ERR_INVALID, "cap_instances %d outside 1 .. %d", cap_instances, 1 << 22);
    if (((uintptr_t)d_key & 3) || ((uintptr_t)d_instances & 7) || ((uintptr_t)d_n & 7))
        return fail(c, SCVOD_ERR_INVALID, "d_key must be 4-byte aligned, d_instances and d_n 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->ev.ran ? c->ev.stream : c->stream);
    if (int rc = counter_block(c, &c->in_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->in, in_work_bytes(cap_instances))) return rc;
    if (int e = launch_instance_score(d_key, d_point_result, (int32_t)n, d_instances, cap_instances, d_n, c->in.buf, c->in_counters, c->in_variant, st))
        return fail(c, SCVOD_ERR_HIP, "rocprim radix sort: %s", hipGetErrorString((hipError_t)e));
    HIPCHK(c, hipGetLastError());
    c->in.stream = st;
    c->in.ran = true;
    return SCVOD_OK;
}

int scvod_score_instances_stats(scvod_ctx* c, int64_t* h_out4) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out4) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->in.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_score_instances_device on this ctx yet");
    if (int rc = read_counters(c, c->in_counters, 4, c->in.stream, h_out4)) return rc;
    if (h_out4[2])
        return fail(c, SCVOD_ERR_CAPACITY, "more distinct keys than cap_instances (at least %lld found)", (long long)h_out4[1]);
    return SCVOD_OK;
}

int64_t scvod_score_instances_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->in.cap + (c->in_counters ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

int scvod_set_score_instances_variant(scvod_ctx* c, int32_t variant) {
    if (!c) return SCVOD_ERR_INVALID;
    if (variant != 0 && variant != 1) return fail(c, SCVOD_ERR_INVALID, "variant %d (0 or 1)", variant);
    c->in_variant = variant;
    return SCVOD_OK;
}

// ---- the truth label every object of the table covers (scvod_objtruth.hip) ----
int scvod_batch_object_truth(scvod_ctx* c, const uint32_t* d_gt_label, const scvod_eval_params* params, void* d_truth, int64_t cap_truth,
                             void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!d_gt_label || !d_truth || cap_truth < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (((uintptr_t)d_gt_label & 3) || ((uintptr_t)d_truth & 3)) return fail(c, SCVOD_ERR_INVALID, "d_gt_label and d_truth must be 4-byte aligned");
    scvod_eval_params p;
    if (params)
        p = *params;
    else
        scvod_eval_params_default(&p);
    if (p.n_dynamic_classes < 0 || p.n_dynamic_classes > 16) return fail(c, SCVOD_ERR_INVALID, "%d dynamic classes (0..16)", p.n_dynamic_classes);
    if (!c->obj_lists_serial) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_truth needs a scvod_batch_objects that asked for records or members");
    if (int rc = export_check(c, c->obj_lists_track, "scvod_batch_object_truth")) return rc;
    if (c->obj_lists_serial != c->cluster_serial)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_truth: the last object table belongs to an earlier clustering: call scvod_batch_objects again");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    if (int rc = counter_block(c, &c->ot_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->ot, truth_work_bytes(c->A.total_pts, c->A.max_scan_pts))) return rc;
    const size_t N = (size_t)(c->cap_pts > 0 ? c->cap_pts : 1);
    TruthJob J{};
    J.tab_stats = c->obj_stats;  // what the table left in the scratch; none of its caller's buffers
    J.key_out = c->obj_keys + N;
    J.begin = c->obj_words + 2 * N;
    J.gt = d_gt_label;
    J.K.n = p.n_dynamic_classes;
    for (int k = 0; k < J.K.n; ++k) J.K.c[k] = p.dynamic_classes[k];
    J.out = (scvod_object_truth*)d_truth;
    J.cap = (long long)cap_truth;
    J.counters = c->ot_counters;
    launch_object_truth(c->A, J, c->ot.buf, st);
    HIPCHK(c, hipGetLastError());
    c->ot.stream = st;
    c->ot.ran = true;
    return SCVOD_OK;
}

int scvod_batch_object_truth_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->ot.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_batch_object_truth on this ctx yet");
    if (int rc = read_counters(c, c->ot_counters, 8, c->ot.stream, h_out8)) return rc;
    if (h_out8[2]) return fail(c, SCVOD_ERR_CAPACITY, "the table holds %lld objects, the truth buffer %lld", (long long)h_out8[1], (long long)h_out8[0]);
    return SCVOD_OK;
}

// internal bridge for scvod_mapfilter.hip (not part of the public header): the lists the last scvod_batch_objects left in the scratch,
// under the state rules of scvod_batch_object_truth; on a refusal *err is the ctx's message
int scvod__ctx_object_lists(scvod_ctx* c, const char* who, const long long** tab_stats, const uint64_t** key_out, const int32_t** begin,
                            const char** err) {
    int rc = SCVOD_OK;
    if (!c->obj_lists_serial)
        rc = fail(c, SCVOD_ERR_STATE, "%s needs a scvod_batch_objects that asked for records or members", who);
    else if ((rc = export_check(c, c->obj_lists_track, who)) != SCVOD_OK)
        ;
    else if (c->obj_lists_serial != c->cluster_serial)
        rc = fail(c, SCVOD_ERR_STATE, "%s: the last object table belongs to an earlier clustering: call scvod_batch_objects again", who);
    *err = c->err.c_str();
    if (rc) return rc;
    const size_t N = (size_t)(c->cap_pts > 0 ? c->cap_pts : 1);
    *tab_stats = c->obj_stats;
    *key_out = c->obj_keys + N;
    *begin = c->obj_words + 2 * N;
    return SCVOD_OK;
}

int64_t scvod_batch_object_truth_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->ot.cap + (c->ot_counters ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

// ---- the ESF descriptor of grouped points and of the table's objects (scvod_objesf.hip) ----
void scvod_esf_params_default(scvod_esf_params* p) {
    if (!p) return;
    p->samples = 20000;  // pcl::ESFEstimation's sample count
    p->seed = 0u;
    p->min_points = 3;
    p->cls_mask = 0xFFFFFFFFu;
    for (int k = 0; k < 4; ++k) p->reserved[k] = 0;
}

// arguments of both forms, before any device is looked for
static int esf_check(scvod_ctx* c, const scvod_esf_params* params, const void* d_records, const float* d_sig640, int64_t cap,
                     scvod_esf_params* p) {
    if (!d_records || cap < 0) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (((uintptr_t)d_records & 3) || ((uintptr_t)d_sig640 & 3)) return fail(c, SCVOD_ERR_INVALID, "d_records and d_sig640 must be 4-byte aligned");
    if (params)
        *p = *params;
    else
        scvod_esf_params_default(p);
    if (p->samples < 1 || p->samples > 65536) return fail(c, SCVOD_ERR_INVALID, "ESF: %d samples (1..65536)", p->samples);
    if (p->min_points < 3) return fail(c, SCVOD_ERR_INVALID, "ESF: min_points %d (at least 3)", p->min_points);
    return SCVOD_OK;
}

// the stage's counters and its block: [pts_bytes: gathered members][cls_bytes: classes][the workgroups' sample bytes]
static int esf_reserve(scvod_ctx* c, const scvod_esf_params& p, size_t pts_bytes, size_t cls_bytes) {
    if (!c->esf_blocks) {
        int cus = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->esf_blocks = 2 * (cus > 0 ? cus : 1);
    }
    if (int rc = counter_block(c, &c->esf_counters, 16)) return rc;
    return scratch_reserve(c, c->esf, pts_bytes + cls_bytes + esf_work_bytes(c->esf_blocks, p.samples));
}

// the calls of a ctx share the counters and the block: one on another stream than the last waits for it on the device
static int esf_order(scvod_ctx* c, hipStream_t st) {
    if (!c->esf.ran || c->esf.stream == st) return SCVOD_OK;
    if (!c->esf_ev) HIPCHK(c, hipEventCreateWithFlags(&c->esf_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->esf_ev, c->esf.stream));
    HIPCHK(c, hipStreamWaitEvent(st, c->esf_ev, 0));
    return SCVOD_OK;
}

static void esf_job(scvod_ctx* c, const scvod_esf_params& p, void* d_records, float* d_sig640, int64_t cap, size_t bytes_off, EsfJob* J) {
    J->samples = p.samples;
    J->min_points = p.min_points;
    J->seed = p.seed;
    J->out = (ObjEsf*)d_records;
    J->sig = d_sig640;
    J->cap = (long long)cap;
    J->sample_bytes = (uint8_t*)c->esf.buf + bytes_off;
    J->counters = c->esf_counters;
    J->blocks = c->esf_blocks;
}

int scvod_esf_device(scvod_ctx* c, const float* d_xyzi, const int32_t* d_begin, int64_t n_objects, const scvod_esf_params* params,
                     void* d_records, float* d_sig640, int64_t cap, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_objects < 0 || (n_objects > 0 && (!d_xyzi || !d_begin))) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (((uintptr_t)d_xyzi & 15) || ((uintptr_t)d_begin & 3)) return fail(c, SCVOD_ERR_INVALID, "d_xyzi must be 16-byte and d_begin 4-byte aligned");
    scvod_esf_params p;
    if (int rc = esf_check(c, params, d_records, d_sig640, cap, &p)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (int rc = esf_reserve(c, p, 0, 0)) return rc;
    if (int rc = esf_order(c, st)) return rc;
    EsfJob J{};
    J.pts = (const float4*)d_xyzi;
    J.begin = d_begin;
    J.n_host = (long long)n_objects;
    J.cls_mask = 0xFFFFFFFFu;
    esf_job(c, p, d_records, d_sig640, cap, 0, &J);
    launch_esf(J, st);
    HIPCHK(c, hipGetLastError());
    c->esf.stream = st;
    c->esf.ran = true;
    return SCVOD_OK;
}

int scvod_batch_object_esf(scvod_ctx* c, const scvod_esf_params* params, void* d_records, float* d_sig640, int64_t cap, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    scvod_esf_params p;
    if (int rc = esf_check(c, params, d_records, d_sig640, cap, &p)) return rc;
    if (!c->obj_lists_serial) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_esf needs a scvod_batch_objects that asked for records or members");
    if (int rc = export_check(c, c->obj_lists_track, "scvod_batch_object_esf")) return rc;
    if (c->obj_lists_serial != c->cluster_serial)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_esf: the last object table belongs to an earlier clustering: call scvod_batch_objects again");
    if (c->obj_lists_types_serial != c->types_serial)  // (cls_mask selects by the class bytes: they must be those the table's records show)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_esf: scvod_batch_cluster_types ran since the last object table: call scvod_batch_objects again");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    const size_t N = (size_t)(c->cap_pts > 0 ? c->cap_pts : 1);
    const size_t M = (size_t)(c->A.total_pts > 0 ? c->A.total_pts : 1);  // (the members are points of this batch)
    const size_t pts_bytes = M * sizeof(float4), cls_bytes = align_up(M, 256);
    if (int rc = esf_reserve(c, p, pts_bytes, cls_bytes)) return rc;
    if (int rc = esf_order(c, st)) return rc;
    float4* pts = (float4*)c->esf.buf;
    uint8_t* cls = (uint8_t*)c->esf.buf + pts_bytes;
    const uint64_t* key_out = c->obj_keys + N;  // what the table left in the scratch; none of its caller's buffers
    const int32_t* begin = c->obj_words + 2 * N;
    launch_esf_gather(c->A, key_out, begin, c->obj_stats, c->rg_done ? c->rg.cls : c->A.pt_type, pts, cls, st);
    EsfJob J{};
    J.pts = pts;
    J.begin = begin;
    J.n_dev = c->obj_stats;
    J.obj_cls = cls;
    J.cls_mask = p.cls_mask;
    esf_job(c, p, d_records, d_sig640, cap, pts_bytes + cls_bytes, &J);
    launch_esf(J, st);
    HIPCHK(c, hipGetLastError());
    c->esf.stream = st;
    c->esf.ran = true;
    return SCVOD_OK;
}

int scvod_esf_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->esf.ran) return fail(c, SCVOD_ERR_STATE, "no ESF call on this ctx yet");
    if (int rc = read_counters(c, c->esf_counters, 8, c->esf.stream, h_out8)) return rc;
    h_out8[7] = 0;
    if (h_out8[3]) return fail(c, SCVOD_ERR_CAPACITY, "%lld objects, the ESF buffer holds %lld", (long long)h_out8[1], (long long)h_out8[0]);
    return SCVOD_OK;
}

int64_t scvod_esf_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->esf.cap + (c->esf_counters ? (int64_t)sizeof(unsigned long long) * 16 : 0) : 0;
}

void scvod_esf_fold10(const float* sig640, float* out10) {
    if (!sig640 || !out10) return;
    for (int j = 0; j < 10; ++j) out10[j] = esf_fold(sig640, j);
}

// SSC::getFeature21 (ssc.cpp:788-795): the 11-value row, then the ten folded ESF values
void scvod_feature_row21(const scvod_object* o, const scvod_object_shape* shape, const scvod_object_esf* esf, double* out21) {
    if (!o || !esf || !out21) return;
    scvod_feature_row(o, shape, out21);
    for (int k = 0; k < 10; ++k) out21[11 + k] = (double)esf->fold10[k];
}

// ---- the objects of the table vote on the seen-through verdict (scvod_objvis.hip) ----
void scvod_object_visibility_params_default(scvod_object_visibility_params* p) {
    if (!p) return;
    p->flags = 0;
    p->min_points = 1;
    p->min_tested = 1;
    p->min_through = 2;
    p->vote_num = 1;
    p->vote_den = 2;
    p->reserved[0] = p->reserved[1] = 0;
}

int scvod_batch_object_visibility(scvod_ctx* c, const uint8_t* d_verdict, const uint32_t* d_votes, const void* d_objects,
                                  const scvod_object_visibility_params* params, void* d_records, int64_t cap_records, uint8_t* d_verdict_out,
                                  void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    scvod_object_visibility_params p;
    if (params)
        p = *params;
    else
        scvod_object_visibility_params_default(&p);
    if (!d_verdict) return fail(c, SCVOD_ERR_INVALID, "NULL d_verdict");
    if (p.flags & ~(SCVOD_OBJVIS_POOL_PAIRS | SCVOD_OBJVIS_WITH_TRACK)) return fail(c, SCVOD_ERR_INVALID, "unknown flag bit (flags %d)", p.flags);
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return fail(c, SCVOD_ERR_INVALID, "scvod_object_visibility_params::reserved must be 0");
    if (p.min_points < 1 || p.min_tested < 1) return fail(c, SCVOD_ERR_INVALID, "min_points %d, min_tested %d: both at least 1", p.min_points, p.min_tested);
    if (p.vote_den < 1 || p.vote_den > (1 << 20) || p.vote_num < 0 || p.vote_num > (1 << 20))
        return fail(c, SCVOD_ERR_INVALID, "vote %d / %d: 0 <= vote_num <= 2^20, 1 <= vote_den <= 2^20", p.vote_num, p.vote_den);
    const bool pool = (p.flags & SCVOD_OBJVIS_POOL_PAIRS) != 0, with_track = (p.flags & SCVOD_OBJVIS_WITH_TRACK) != 0;
    if (pool && !d_votes) return fail(c, SCVOD_ERR_INVALID, "SCVOD_OBJVIS_POOL_PAIRS without d_votes");
    if (with_track && !d_objects) return fail(c, SCVOD_ERR_INVALID, "SCVOD_OBJVIS_WITH_TRACK without d_objects");
    if (cap_records < 0) return fail(c, SCVOD_ERR_INVALID, "cap_records below 0");
    if (((uintptr_t)d_votes & 3u) || ((uintptr_t)d_records & 3u)) return fail(c, SCVOD_ERR_INVALID, "d_votes and d_records must be 4-byte aligned");
    if ((uintptr_t)d_objects & 7u) return fail(c, SCVOD_ERR_INVALID, "d_objects is not 8-byte aligned");
    if (d_verdict_out && d_verdict_out != d_verdict) {
        const uintptr_t n = (uintptr_t)(c->batch_valid && c->A.total_pts > 0 ? c->A.total_pts : 0);
        const uintptr_t o0 = (uintptr_t)d_verdict_out, o1 = o0 + n;
        auto hits = [&](const void* q, uintptr_t bytes) { return q && bytes > 0 && o0 < (uintptr_t)q + bytes && (uintptr_t)q < o1; };
        const uintptr_t recs = (uintptr_t)(cap_records > 0 ? cap_records : 0);
        if (n > 0 && (hits(d_verdict, n) || hits(d_votes, 4 * n) || hits(d_records, sizeof(scvod_object_visibility) * recs) ||
                      hits(d_objects, sizeof(scvod_object) * (recs > 0 ? recs : 1))))
            return fail(c, SCVOD_ERR_INVALID, "d_verdict_out overlaps an input or d_records (only d_verdict_out == d_verdict works in place)");
    }
    const long long* tab_stats = nullptr;
    const uint64_t* key_out = nullptr;
    const int32_t* begin = nullptr;
    const char* why = "";
    if (int rc = scvod__ctx_object_lists(c, "scvod_batch_object_visibility", &tab_stats, &key_out, &begin, &why)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    if (int rc = counter_block(c, &c->ov_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->ov, objvis_work_bytes(c->A.total_pts))) return rc;
    ObjVisJob J{};
    J.tab_stats = tab_stats;  // what the table left in the scratch; of its caller's buffers d_objects alone, and only with WITH_TRACK
    J.key_out = key_out;
    J.begin = begin;
    J.verdict = d_verdict;
    J.votes = d_votes;
    J.obj_bytes = with_track ? (const unsigned char*)d_objects : nullptr;
    J.out = d_verdict_out;
    J.rec = (scvod_object_visibility*)d_records;
    J.cap = (long long)cap_records;
    J.pool = pool ? 1 : 0;
    J.min_points = p.min_points;
    J.min_tested = p.min_tested;
    J.min_through = p.min_through;
    J.vote_num = p.vote_num;
    J.vote_den = p.vote_den;
    J.counters = c->ov_counters;
    launch_object_visibility(c->A, J, c->ov.buf, st);
    HIPCHK(c, hipGetLastError());
    c->ov.stream = st;
    c->ov.ran = true;
    return SCVOD_OK;
}

int scvod_batch_object_visibility_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->ov.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_batch_object_visibility on this ctx yet");
    if (int rc = read_counters(c, c->ov_counters, 8, c->ov.stream, h_out8)) return rc;
    if (h_out8[7]) return fail(c, SCVOD_ERR_CAPACITY, "the table holds %lld objects, the record buffer %lld", (long long)h_out8[0], (long long)h_out8[6]);
    return SCVOD_OK;
}

int64_t scvod_batch_object_visibility_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->ov.cap + (c->ov_counters ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

// ---- the objects of a table linked into tracks (scvod_tracks.hip) ----
// what both forms refuse before a device is touched; *p receives the parameters in force
static int trk_check(scvod_ctx* c, const scvod_track_params* params, scvod_track_params* p, const void* d_objects, const void* d_links,
                     int64_t cap_links, const void* d_tracks, int64_t cap_tracks, const void* d_track_objects, const void* d_n_tracks) {
    if (params)
        *p = *params;
    else
        scvod_track_params_default(p);
    if (p->flags & ~(SCVOD_TRK_NO_GATE | SCVOD_TRK_ANY_CLASS)) return fail(c, SCVOD_ERR_INVALID, "unknown flag bit (flags %d)", p->flags);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(c, SCVOD_ERR_INVALID, "scvod_track_params::reserved must be 0");
    if (p->occupancy != p->occupancy) return fail(c, SCVOD_ERR_INVALID, "occupancy is NaN");
    if (!(p->gate > 0.f) || !std::isfinite(p->gate)) return fail(c, SCVOD_ERR_INVALID, "gate %g: a positive finite number of metres", (double)p->gate);
    if (!(p->size_ratio >= 1.f)) return fail(c, SCVOD_ERR_INVALID, "size_ratio %g below 1", (double)p->size_ratio);
    if (p->min_points < 1 || p->min_length < 1)
        return fail(c, SCVOD_ERR_INVALID, "min_points %d, min_length %d: both at least 1", p->min_points, p->min_length);
    if (cap_links < 0 || cap_tracks < 0 || cap_links > 2147483647ll) return fail(c, SCVOD_ERR_INVALID, "cap_links %lld / cap_tracks %lld", (long long)cap_links, (long long)cap_tracks);
    if (cap_links > 0 && !d_objects) return fail(c, SCVOD_ERR_INVALID, "NULL d_objects with cap_links %lld", (long long)cap_links);
    if ((uintptr_t)d_objects & 7u) return fail(c, SCVOD_ERR_INVALID, "d_objects is not 8-byte aligned");
    if (((uintptr_t)d_links & 3u) || ((uintptr_t)d_tracks & 3u) || ((uintptr_t)d_track_objects & 3u) || ((uintptr_t)d_n_tracks & 3u))
        return fail(c, SCVOD_ERR_INVALID, "d_links, d_tracks, d_track_objects and d_n_tracks must be 4-byte aligned");
    if (p->occupancy < 0.f) p->occupancy = c->params.occupancy;
    return SCVOD_OK;
}

// the successor table of n_scans scans under scvod_visibility_viewers' rules -> next (negative: none)
static int trk_next_table(scvod_ctx* c, const int32_t* h_next_scan, int n_scans, std::vector<int32_t>& next) {
    std::vector<int32_t> begin, viewers;
    if (vis_viewers(h_next_scan, n_scans, 0, 1, begin, viewers))
        return fail(c, SCVOD_ERR_INVALID, "object tracks: the successor table names a scan outside the batch, a scan itself, one successor twice or a ring");
    next.resize((size_t)n_scans);
    for (int s = 0; s < n_scans; ++s) {
        const int32_t v = h_next_scan ? h_next_scan[s] : (s + 1 < n_scans ? s + 1 : -1);
        next[s] = v < 0 ? -1 : v;
    }
    return SCVOD_OK;
}

static int trk_run(scvod_ctx* c, TrkJob J, const std::vector<int32_t>& next, const float* h_poses, const int32_t* scan_cnt, hipStream_t st) {
    const size_t B = (size_t)J.n_scans, b_T = align_up(sizeof(float) * 12 * B, 256), b_tab = b_T + sizeof(int32_t) * B;
    c->trk_host.assign(b_tab > 0 ? b_tab : 1, 0);
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t s = 0; s < B; ++s) scvod_pose_matrix(h_poses ? h_poses + 6 * s : zero, (float*)c->trk_host.data() + 12 * s);
    if (B) memcpy(c->trk_host.data() + b_T, next.data(), sizeof(int32_t) * B);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = counter_block(c, &c->trk_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->trk, trk_work_bytes(J.cap, J.n_scans))) return rc;  // (waits for the call in flight before the block moves)
    c->trk.stream = st;
    c->trk.ran = true;
    HIPCHK(c, hipMemsetAsync(c->trk_counters, 0, 8 * sizeof(unsigned long long), st));
    if (B)
        if (int rc = staged_upload(c, c->trk_host.data(), b_tab, c->trk.buf, st)) return rc;
    J.counters = c->trk_counters;
    const hipError_t e = launch_object_tracks(c->A, J, scan_cnt, c->trk.buf, st);
    if (e != hipSuccess) return fail(c, SCVOD_ERR_HIP, "object tracks: %s", hipGetErrorString(e));
    return SCVOD_OK;
}

static void trk_fill(TrkJob& J, const scvod_track_params& p, const void* d_objects, void* d_links, int64_t cap_links, void* d_tracks,
                     int64_t cap_tracks, int32_t* d_track_objects, int32_t* d_n_tracks) {
    J.objects = (const scvod_object*)d_objects;
    J.cap = (long long)cap_links;
    J.flags = p.flags;
    J.min_points = p.min_points;
    J.min_length = p.min_length;
    J.occupancy = p.occupancy;
    J.gate2 = p.gate * p.gate;
    J.size_ratio = p.size_ratio;
    J.out_links = (scvod_object_link*)d_links;
    J.out_tracks = (scvod_track*)d_tracks;
    J.cap_tracks = (long long)cap_tracks;
    J.out_tobj = d_track_objects;
    J.n_tracks = d_n_tracks;
}

int scvod_object_tracks_device(scvod_ctx* c, const void* d_objects, const int32_t* d_obj_offsets, int32_t n_scans, const int32_t* h_next_scan,
                               const float* h_poses, const int32_t* d_cand_begin, const void* d_cand, const scvod_track_params* params,
                               void* d_links, int64_t cap_links, void* d_tracks, int64_t cap_tracks, int32_t* d_track_objects,
                               int32_t* d_n_tracks, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    scvod_track_params p;
    if (int rc = trk_check(c, params, &p, d_objects, d_links, cap_links, d_tracks, cap_tracks, d_track_objects, d_n_tracks)) return rc;
    if (n_scans < 0) return fail(c, SCVOD_ERR_INVALID, "n_scans below 0");
    if (!d_obj_offsets || ((uintptr_t)d_obj_offsets & 3u)) return fail(c, SCVOD_ERR_INVALID, "d_obj_offsets is NULL or not 4-byte aligned");
    if (d_cand && !d_cand_begin) return fail(c, SCVOD_ERR_INVALID, "d_cand without d_cand_begin");
    if (((uintptr_t)d_cand & 7u) || ((uintptr_t)d_cand_begin & 3u)) return fail(c, SCVOD_ERR_INVALID, "d_cand must be 8-byte, d_cand_begin 4-byte aligned");
    std::vector<int32_t> next;
    if (int rc = trk_next_table(c, h_next_scan, n_scans, next)) return rc;
    TrkJob J{};
    trk_fill(J, p, d_objects, d_links, cap_links, d_tracks, cap_tracks, d_track_objects, d_n_tracks);
    J.obj_off = d_obj_offsets;
    J.n_scans = n_scans;
    J.cand_begin = d_cand ? d_cand_begin : nullptr;
    J.cand = (const int2*)d_cand;
    return trk_run(c, J, next, h_poses, nullptr, stream ? (hipStream_t)stream : c->stream);
}

int scvod_batch_object_tracks(scvod_ctx* c, const void* d_objects, const float* h_poses, const scvod_track_params* params, void* d_links,
                              int64_t cap_links, void* d_tracks, int64_t cap_tracks, int32_t* d_track_objects, int32_t* d_n_tracks,
                              void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    scvod_track_params p;
    if (int rc = trk_check(c, params, &p, d_objects, d_links, cap_links, d_tracks, cap_tracks, d_track_objects, d_n_tracks)) return rc;
    if (!d_objects) return fail(c, SCVOD_ERR_INVALID, "NULL d_objects");
    const long long* tab_stats = nullptr;
    const uint64_t* key_out = nullptr;
    const int32_t* begin = nullptr;
    const char* why = "";
    if (!c->obj_lists_serial) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_tracks needs a scvod_batch_objects that asked for records or members");
    if (!c->obj_lists_track) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_tracks: the table was made with SCVOD_OBJ_NO_TRACK");
    if (!c->track_valid) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_tracks needs a current scvod_batch_track");
    if (int rc = scvod__ctx_object_lists(c, "scvod_batch_object_tracks", &tab_stats, &key_out, &begin, &why)) return rc;
    const int B = c->A.n_scans;
    if ((int)c->up_next.size() != B) return fail(c, SCVOD_ERR_STATE, "scvod_batch_object_tracks: the ctx holds no successor table of this batch");
    std::vector<int32_t> next;
    if (int rc = trk_next_table(c, c->up_next.data(), B, next)) return rc;
    TrkJob J{};
    trk_fill(J, p, d_objects, d_links, cap_links, d_tracks, cap_tracks, d_track_objects, d_n_tracks);
    J.n_scans = B;
    J.root_obj = c->obj_words;  // what the table left in its scratch, read only
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    return trk_run(c, J, next, h_poses, c->obj_scan_cnt, st);
}

int scvod_object_tracks_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->trk.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_object_tracks_device / scvod_batch_object_tracks on this ctx yet");
    if (int rc = read_counters(c, c->trk_counters, 8, c->trk.stream, h_out8)) return rc;
    if (h_out8[7])
        return fail(c, SCVOD_ERR_CAPACITY, "object tracks: %lld objects, %lld listed tracks, %lld track records written: a capacity was too small",
                    (long long)h_out8[0], (long long)h_out8[1], (long long)h_out8[2]);
    return SCVOD_OK;
}

int64_t scvod_object_tracks_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->trk.cap + (c->trk_counters ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

// ---- the tracks of a table vote on the seen-through verdict (scvod_trackvis.hip) ----
int scvod_track_visibility_device(scvod_ctx* c, const void* d_objects, const int32_t* d_obj_offsets, int32_t n_scans, const float* h_poses,
                                  const void* d_links, int64_t cap_objects, const void* d_tracks, int64_t cap_tracks,
                                  const int32_t* d_track_objects, const int32_t* d_n_tracks, const void* d_object_vis,
                                  const int32_t* d_point_object, const uint8_t* d_verdict, uint8_t* d_verdict_out, int64_t n_points,
                                  const scvod_track_visibility_params* params, void* d_track_votes, int64_t cap_track_votes,
                                  void* d_object_votes, int64_t cap_object_votes, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    scvod_track_visibility_params p;
    if (params)
        p = *params;
    else
        scvod_track_visibility_params_default(&p);
    if (p.flags & ~(SCVOD_TRKVIS_NO_DYNAMIC | SCVOD_TRKVIS_CLEAR)) return fail(c, SCVOD_ERR_INVALID, "unknown flag bit (flags %d)", p.flags);
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return fail(c, SCVOD_ERR_INVALID, "scvod_track_visibility_params::reserved must be 0");
    if (p.window < 0) return fail(c, SCVOD_ERR_INVALID, "window %d below 0", p.window);
    if (!(p.min_travel > 0.f) || !std::isfinite(p.min_travel))
        return fail(c, SCVOD_ERR_INVALID, "min_travel %g: a positive finite number of metres", (double)p.min_travel);
    if (p.min_length < 1 || p.min_moved < 1) return fail(c, SCVOD_ERR_INVALID, "min_length %d, min_moved %d: both at least 1", p.min_length, p.min_moved);
    if (p.vote_den < 1 || p.vote_den > (1 << 20) || p.vote_num < 0 || p.vote_num > (1 << 20))
        return fail(c, SCVOD_ERR_INVALID, "vote %d / %d: 0 <= vote_num <= 2^20, 1 <= vote_den <= 2^20", p.vote_num, p.vote_den);
    if (n_scans < 0) return fail(c, SCVOD_ERR_INVALID, "n_scans below 0");
    if (cap_objects < 0 || cap_objects > 2147483647ll || cap_tracks < 0 || cap_track_votes < 0 || cap_object_votes < 0 || n_points < 0)
        return fail(c, SCVOD_ERR_INVALID, "cap_objects %lld, cap_tracks %lld, cap_track_votes %lld, cap_object_votes %lld, n_points %lld",
                    (long long)cap_objects, (long long)cap_tracks, (long long)cap_track_votes, (long long)cap_object_votes, (long long)n_points);
    if (!d_obj_offsets || !d_links || !d_tracks || !d_track_objects || !d_n_tracks)
        return fail(c, SCVOD_ERR_INVALID, "NULL d_obj_offsets, d_links, d_tracks, d_track_objects or d_n_tracks");
    if (cap_objects > 0 && !d_objects) return fail(c, SCVOD_ERR_INVALID, "NULL d_objects with cap_objects %lld", (long long)cap_objects);
    if (d_verdict_out && !d_point_object) return fail(c, SCVOD_ERR_INVALID, "d_verdict_out without d_point_object");
    if ((uintptr_t)d_objects & 7u) return fail(c, SCVOD_ERR_INVALID, "d_objects is not 8-byte aligned");
    if (((uintptr_t)d_obj_offsets & 3u) || ((uintptr_t)d_links & 3u) || ((uintptr_t)d_tracks & 3u) || ((uintptr_t)d_track_objects & 3u) ||
        ((uintptr_t)d_n_tracks & 3u) || ((uintptr_t)d_object_vis & 3u) || ((uintptr_t)d_point_object & 3u) || ((uintptr_t)d_track_votes & 3u) ||
        ((uintptr_t)d_object_votes & 3u))
        return fail(c, SCVOD_ERR_INVALID, "every pointer to records or int32 must be 4-byte aligned");
    if (d_verdict_out && n_points > 0) {
        const uintptr_t n = (uintptr_t)n_points, o0 = (uintptr_t)d_verdict_out, o1 = o0 + n;
        const uintptr_t co = (uintptr_t)cap_objects, ct = (uintptr_t)cap_tracks;
        auto hits = [&](const void* q, uintptr_t bytes) { return q && bytes > 0 && o0 < (uintptr_t)q + bytes && (uintptr_t)q < o1; };
        if ((d_verdict_out != d_verdict && hits(d_verdict, n)) || hits(d_point_object, 4 * n) || hits(d_objects, sizeof(scvod_object) * co) ||
            hits(d_obj_offsets, 4 * ((uintptr_t)n_scans + 1)) || hits(d_links, sizeof(scvod_object_link) * co) ||
            hits(d_tracks, sizeof(scvod_track) * ct) || hits(d_track_objects, 4 * co) || hits(d_n_tracks, 4) ||
            hits(d_object_vis, sizeof(scvod_object_visibility) * co) || hits(d_track_votes, sizeof(scvod_track_vote) * (uintptr_t)cap_track_votes) ||
            hits(d_object_votes, sizeof(scvod_object_track_vote) * (uintptr_t)cap_object_votes))
            return fail(c, SCVOD_ERR_INVALID, "d_verdict_out overlaps an input or a record buffer (only d_verdict_out == d_verdict works in place)");
    }
    const size_t B = (size_t)n_scans;
    c->tv_host.assign(12 * B > 0 ? 12 * B : 1, 0.f);
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (size_t s = 0; s < B; ++s) scvod_pose_matrix(h_poses ? h_poses + 6 * s : zero, c->tv_host.data() + 12 * s);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (int rc = counter_block(c, &c->tv_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->tv, tv_work_bytes(cap_objects, cap_tracks, n_scans))) return rc;  // (waits for the call in flight before the block moves)
    c->tv.stream = st;
    c->tv.ran = true;
    HIPCHK(c, hipMemsetAsync(c->tv_counters, 0, 8 * sizeof(unsigned long long), st));
    if (B)
        if (int rc = staged_upload(c, c->tv_host.data(), sizeof(float) * 12 * B, c->tv.buf, st)) return rc;
    TvJob J{};
    J.objects = (const scvod_object*)d_objects;
    J.obj_off = d_obj_offsets;
    J.n_scans = n_scans;
    J.cap = (long long)cap_objects;
    J.links = (const scvod_object_link*)d_links;
    J.tracks = (const scvod_track*)d_tracks;
    J.cap_tracks = (long long)cap_tracks;
    J.tobj = d_track_objects;
    J.n_tracks = d_n_tracks;
    J.ovis = (const scvod_object_visibility*)d_object_vis;
    J.point_object = d_point_object;
    J.verdict = d_verdict;
    J.out = d_point_object ? d_verdict_out : nullptr;
    J.n_points = (long long)n_points;
    J.flags = p.flags;
    J.window = p.window;
    J.min_length = p.min_length;
    J.min_moved = p.min_moved;
    J.min_flagged = p.min_flagged;
    J.vote_num = p.vote_num;
    J.vote_den = p.vote_den;
    J.travel2_min = p.min_travel * p.min_travel;
    J.out_tracks = (scvod_track_vote*)d_track_votes;
    J.cap_tvotes = (long long)cap_track_votes;
    J.out_objs = (scvod_object_track_vote*)d_object_votes;
    J.cap_ovotes = (long long)cap_object_votes;
    J.counters = c->tv_counters;
    const hipError_t e = launch_track_visibility(J, c->tv.buf, st);
    if (e != hipSuccess) return fail(c, SCVOD_ERR_HIP, "track visibility: %s", hipGetErrorString(e));
    return SCVOD_OK;
}

int scvod_track_visibility_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->tv.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_track_visibility_device on this ctx yet");
    if (int rc = read_counters(c, c->tv_counters, 8, c->tv.stream, h_out8)) return rc;
    if (h_out8[7] & 3)
        return fail(c, SCVOD_ERR_CAPACITY, "track visibility: %lld objects, %lld listed tracks: a capacity was too small (latch bits %lld)",
                    (long long)h_out8[0], (long long)h_out8[1], (long long)h_out8[7]);
    return SCVOD_OK;
}

int64_t scvod_track_visibility_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->tv.cap + (c->tv_counters ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

void scvod_object_truth_params_default(scvod_object_truth_params* p) {
    if (!p) return;
    p->moving_from = 0.5;
    p->pure_from = 0.5;
    p->min_points = 1;
}

int scvod_object_truth_finish(const scvod_object* objects, const scvod_object_truth* truth, int64_t n, const scvod_object_truth_params* params,
                              scvod_object_truth_result* out) {
    if (n < 0 || (n > 0 && (!objects || !truth)) || !out) return SCVOD_ERR_INVALID;
    scvod_object_truth_params p;
    if (params)
        p = *params;
    else
        scvod_object_truth_params_default(&p);
    if (!std::isfinite(p.moving_from) || !std::isfinite(p.pure_from)) return SCVOD_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    for (int64_t i = 0; i < n; ++i) {
        const scvod_object& o = objects[i];
        const scvod_object_truth& t = truth[i];
        if ((int64_t)t.n_points < p.min_points) {
            ++out->skipped;
            continue;
        }
        if ((double)t.n_label < p.pure_from * (double)t.n_points) ++out->mixed_objects;
        if ((double)t.n_moving >= p.moving_from * (double)t.n_points) {
            ++out->moving_objects;
            if (o.dynamic == 1)
                ++out->moving_dynamic;
            else if (o.cls != 2)
                ++out->moving_not_car;
            else if (o.state == 0)
                ++out->moving_car_static;
            else
                ++out->moving_car_untracked;
        } else {
            ++out->static_objects;
            if (o.dynamic == 1) ++out->static_dynamic;
        }
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();  // scvod_eval_finish's rule for a zero denominator
    const int64_t alarms = out->moving_dynamic + out->static_dynamic;
    out->precision = alarms ? 100.0 * (double)out->moving_dynamic / (double)alarms : nan;
    out->recall = out->moving_objects ? 100.0 * (double)out->moving_dynamic / (double)out->moving_objects : nan;
    return SCVOD_OK;
}

// ---- scan stacking (scvod_stack.hip) ----
int scvod_batch_stack_scans(scvod_ctx* c, const void* d_xyzi_in, const int32_t* h_in_offsets, int32_t n_in, const float* h_poses, int32_t window,
                            int32_t interval, int32_t flags, const uint32_t* d_payload_in, void* d_xyzi_out, uint32_t* d_payload_out,
                            int32_t* d_src_out, int64_t cap_points, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_in < 0 || cap_points < 0 || !h_in_offsets) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (h_in_offsets[0] < 0) return fail(c, SCVOD_ERR_INVALID, "scan offsets must not start below 0");
    const int n_out = scvod_stack_offsets(h_in_offsets, n_in, window, interval, flags, nullptr, nullptr, 0, nullptr);
    if (n_out == SCVOD_ERR_INVALID)
        return fail(c, SCVOD_ERR_INVALID, "scvod_batch_stack_scans: window %d must be odd and 1..%d, interval %d >= 1, flags %d 0 or SCVOD_STACK_REFERENCE_BOUND, offsets ascending",
                    window, SCVOD_STACK_MAX_WINDOW, interval, flags);
    if (d_payload_out && !d_payload_in) return fail(c, SCVOD_ERR_INVALID, "a payload output needs a payload input");
    if (((uintptr_t)d_xyzi_in & 15) || ((uintptr_t)d_xyzi_out & 15)) return fail(c, SCVOD_ERR_INVALID, "the xyzi arrays must be 16-byte aligned");
    if (((uintptr_t)d_payload_in & 3) || ((uintptr_t)d_payload_out & 3) || ((uintptr_t)d_src_out & 3))
        return fail(c, SCVOD_ERR_INVALID, "the payload and source index arrays must be 4-byte aligned");
    if (n_out == 0) return SCVOD_OK;
    if (!h_poses) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    // segments in output order: per group the middle scan, then the others ascending; tiles of the non-empty ones
    const size_t n_seg = (size_t)n_out * (size_t)window;
    long long need = 0;
    size_t n_tiles = 0;
    for (int g = 0; g < n_out; ++g) {
        const long long pts = (long long)h_in_offsets[(size_t)g * interval + window] - (long long)h_in_offsets[(size_t)g * interval];
        need += pts;
        for (int k = 0; k < window; ++k) {
            const size_t s = (size_t)g * interval + k;
            n_tiles += (size_t)(((long long)h_in_offsets[s + 1] - h_in_offsets[s] + kStackTile - 1) / kStackTile);
        }
    }
    if (need > 2147483647ll) return fail(c, SCVOD_ERR_CAPACITY, "%lld stacked points outgrow int32 offsets", need);
    if (need > cap_points) return fail(c, SCVOD_ERR_CAPACITY, "%lld stacked points, the output holds %lld", need, (long long)cap_points);
    if (need == 0) return SCVOD_OK;
    if (n_tiles > 2147483647ull) return fail(c, SCVOD_ERR_CAPACITY, "too many tiles");
    if (!d_xyzi_in || !d_xyzi_out) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    {  // an output range must not meet the range it is made from (the overlapping windows of interval < window read a scan repeatedly)
        const long long lo = h_in_offsets[0], hi = h_in_offsets[n_in];
        auto meets = [](const void* a, long long a_bytes, const void* b, long long b_bytes) {
            const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
            return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
        };
        if (meets(d_xyzi_out, 16 * need, (const char*)d_xyzi_in + 16 * lo, 16 * (hi - lo)))
            return fail(c, SCVOD_ERR_INVALID, "the xyzi output overlaps the xyzi input");
        if (d_payload_out && meets(d_payload_out, 4 * need, (const char*)d_payload_in + 4 * lo, 4 * (hi - lo)))
            return fail(c, SCVOD_ERR_INVALID, "the payload output overlaps the payload input");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const size_t off_tiles = sizeof(StackSeg) * n_seg, bytes = off_tiles + sizeof(StackTile) * n_tiles;
    c->stk_host.resize(bytes);
    StackSeg* segs = (StackSeg*)c->stk_host.data();
    StackTile* tiles = (StackTile*)(c->stk_host.data() + off_tiles);
    size_t seg = 0, tile = 0;
    long long out = 0;
    for (int g = 0; g < n_out; ++g) {
        const int first = g * interval, mid = first + window / 2;
        for (int j = 0; j < window; ++j) {
            // j = 0: the middle scan; then the scans of the window in ascending index, the middle one left out
            const int k = j == 0 ? mid : (first + j - 1 < mid ? first + j - 1 : first + j);
            StackSeg& S = segs[seg];
            memset(&S, 0, sizeof(S));
            S.in_base = h_in_offsets[k];
            S.out_base = (int32_t)out;
            S.n = h_in_offsets[k + 1] - h_in_offsets[k];
            S.copy = k == mid ? 1 : 0;
            if (!S.copy) scvod_pose_delta(h_poses + 6 * (size_t)k, h_poses + 6 * (size_t)mid, S.T);  // trans_mid^-1 * trans_k
            for (int i = 0; i < S.n; i += kStackTile) tiles[tile++] = StackTile{(int32_t)seg, i};
            out += S.n;
            ++seg;
        }
    }
    if (int rc = scratch_reserve(c, c->stk, bytes)) return rc;  // (the old tables may still be read by a stacking call in flight)
    if (int rc = staged_upload(c, c->stk_host.data(), bytes, c->stk.buf, st)) return rc;
    launch_stack((const StackSeg*)c->stk.buf, (const StackTile*)((const unsigned char*)c->stk.buf + off_tiles), (int)n_tiles,
                 (const float4*)d_xyzi_in, (float4*)d_xyzi_out, d_payload_in, d_payload_out, d_src_out, st);
    HIPCHK(c, hipGetLastError());
    c->stk.stream = st;
    c->stk.ran = true;
    return SCVOD_OK;
}

int scvod_stack_scans(scvod_ctx* c, const float* h_xyzi_in, const int32_t* h_in_offsets, int32_t n_in, const float* h_poses, int32_t window,
                      int32_t interval, int32_t flags, float* h_xyzi_out, int64_t cap_points) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_in < 0 || cap_points < 0 || !h_in_offsets) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (h_in_offsets[0] < 0) return fail(c, SCVOD_ERR_INVALID, "scan offsets must not start below 0");
    int32_t largest = 0;
    const int n_out = scvod_stack_offsets(h_in_offsets, n_in, window, interval, flags, nullptr, nullptr, 0, &largest);
    if (n_out < 0) return fail(c, n_out, "scvod_stack_scans: bad window %d / interval %d / flags %d / offsets", window, interval, flags);
    long long need = 0;
    for (int g = 0; g < n_out; ++g) need += (long long)h_in_offsets[(size_t)g * interval + window] - (long long)h_in_offsets[(size_t)g * interval];
    if (need > cap_points) return fail(c, SCVOD_ERR_CAPACITY, "%lld stacked points, the output holds %lld", need, (long long)cap_points);
    if (need == 0) return SCVOD_OK;
    if (!h_xyzi_in || !h_xyzi_out || !h_poses) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const long long lo = h_in_offsets[0], n_pts = (long long)h_in_offsets[n_in] - lo;
    std::vector<int32_t> off((size_t)n_in + 1);
    for (int k = 0; k <= n_in; ++k) off[k] = h_in_offsets[k] - (int32_t)lo;
    void *d_in = nullptr, *d_out = nullptr;
    int rc = SCVOD_OK;
    if (hipMalloc(&d_in, 16 * (size_t)n_pts) != hipSuccess || hipMalloc(&d_out, 16 * (size_t)need) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_stack_scans: no device memory for %lld + %lld points", n_pts, need);
    if (rc == SCVOD_OK && hipMemcpyAsync(d_in, h_xyzi_in + 4 * lo, 16 * (size_t)n_pts, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_stack_scans: upload failed");
    if (rc == SCVOD_OK)
        rc = scvod_batch_stack_scans(c, d_in, off.data(), n_in, h_poses, window, interval, flags, nullptr, d_out, nullptr, nullptr, need, c->stream);
    if (rc == SCVOD_OK && hipMemcpyAsync(h_xyzi_out, d_out, 16 * (size_t)need, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_stack_scans: download failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == SCVOD_OK) rc = fail(c, SCVOD_ERR_HIP, "scvod_stack_scans: the stream failed");
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    return rc;
}

int64_t scvod_stack_scratch_bytes(scvod_ctx* c) { return c ? (int64_t)c->stk.cap : 0; }

// ---- seen-through points (scvod_visibility.hip) ----
struct VisOut {
    uint32_t* d_votes;
    uint8_t* d_verdict;
    float* d_images;
    int64_t* d_scan_counts;
};

// what both forms refuse before a device is touched
static int vis_check(scvod_ctx* c, const scvod_visibility_params* p, const VisOut& o) {
    if (!p) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (vis_check_params(p))
        return fail(c, SCVOD_ERR_INVALID,
                    "visibility: before %d / after %d must be 0..%d and not both 0, halo %d 0 or 1, vote %d / %d with 0 <= num <= 1 << 20 and 1 <= den <= 1 << 20, gaps %g + %g * dis finite and >= 0",
                    p->before, p->after, SCVOD_VIS_MAX_WINDOW, p->halo, p->vote_num, p->vote_den, (double)p->gap_abs, (double)p->gap_rel);
    if ((uintptr_t)o.d_images & 15) return fail(c, SCVOD_ERR_INVALID, "d_images is not 16-byte aligned");
    if ((uintptr_t)o.d_votes & 3) return fail(c, SCVOD_ERR_INVALID, "d_votes is not 4-byte aligned");
    if ((uintptr_t)o.d_scan_counts & 7) return fail(c, SCVOD_ERR_INVALID, "d_scan_counts is not 8-byte aligned");
    return SCVOD_OK;
}

// the vote over scans [0, n_scans) of a cloud on the device; h_off [n_scans + 1] checked by the caller; with_mask: the batch form, whose
// mask of the non-ground list is scattered into the scratch here
static int vis_run(scvod_ctx* c, const void* d_xyzi, const int32_t* h_off, int n_scans, const float* h_poses, const std::vector<int32_t>& begin,
                   const std::vector<int32_t>& viewers, const uint8_t* d_mask, bool with_mask, const scvod_visibility_params* p, const VisOut& o,
                   hipStream_t st, bool images_only = false) {
    const BinParams& g = c->dev.bin;
    const size_t img_words = (size_t)g.azimuth_num * (size_t)g.sector_num;
    if (g.azimuth_num <= 0 || g.sector_num <= 0) return fail(c, SCVOD_ERR_INVALID, "the ctx's grid has no pixels");
    const long long hi = n_scans > 0 ? h_off[n_scans] : 0;
    size_t n_tiles = 0;
    for (int s = 0; s < n_scans; ++s) n_tiles += (size_t)(((long long)h_off[s + 1] - h_off[s] + kStackTile - 1) / kStackTile);
    if (n_tiles > 2147483647ull) return fail(c, SCVOD_ERR_CAPACITY, "too many tiles");
    const size_t n_pairs = viewers.size();
    // the block: [images unless the caller holds them][pairs][scans][tiles][mask of the batch form]
    const size_t b_img = o.d_images ? 0 : align_up(sizeof(float) * img_words * (size_t)n_scans, 256);
    const size_t b_pairs = align_up(sizeof(VisPair) * n_pairs, 256), b_scans = align_up(sizeof(VisScan) * (size_t)n_scans, 256);
    const size_t b_tiles = align_up(sizeof(StackTile) * n_tiles, 256), b_tab = b_pairs + b_scans + b_tiles;
    const size_t b_mask = with_mask ? align_up((size_t)hi, 256) : 0;
    c->vis_host.assign(b_tab, 0);
    VisPair* pairs = (VisPair*)c->vis_host.data();
    VisScan* scans = (VisScan*)(c->vis_host.data() + b_pairs);
    StackTile* tiles = (StackTile*)(c->vis_host.data() + b_pairs + b_scans);
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    size_t tile = 0;
    for (int j = 0; j < n_scans; ++j) {
        VisScan& S = scans[j];
        S.base = h_off[j];
        S.n = h_off[j + 1] - h_off[j];
        S.pair_begin = begin[j];
        S.n_pairs = begin[(size_t)j + 1] - begin[j];
        for (int k = begin[j]; k < begin[(size_t)j + 1]; ++k) {
            const int v = viewers[k];
            pairs[k].viewer = v;
            // trans_v^-1 * trans_j: a point of j's frame in v's frame (scvod_batch_stack_scans' argument order)
            scvod_pose_delta(h_poses ? h_poses + 6 * (size_t)j : zero, h_poses ? h_poses + 6 * (size_t)v : zero, pairs[k].T);
        }
        for (int i = 0; i < S.n; i += kStackTile) tiles[tile++] = StackTile{(int32_t)j, i};
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = counter_block(c, &c->vis_counters, 8)) return rc;
    if (int rc = scratch_reserve(c, c->vis, b_img + b_tab + b_mask + 256)) return rc;  // (waits for the vote in flight before the block moves)
    unsigned char* blk = (unsigned char*)c->vis.buf;
    c->vis.stream = st;
    c->vis.ran = true;
    HIPCHK(c, hipMemsetAsync(c->vis_counters, 0, 8 * sizeof(unsigned long long), st));
    if (o.d_scan_counts && n_scans > 0) HIPCHK(c, hipMemsetAsync(o.d_scan_counts, 0, 6 * sizeof(int64_t) * (size_t)n_scans, st));
    float* images = o.d_images ? o.d_images : (float*)blk;
    if (n_scans > 0) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)images, 0x7F800000, img_words * (size_t)n_scans, st));  // +inf
    if (n_tiles == 0) return SCVOD_OK;
    if (int rc = staged_upload(c, c->vis_host.data(), b_tab, blk + b_img, st)) return rc;
    if (with_mask) {
        uint8_t* mask = blk + b_img + b_tab;
        if (int rc = ensure_lists(c, st)) return rc;
        HIPCHK(c, hipMemsetAsync(mask, 0, (size_t)hi, st));
        launch_vis_mask(c->A, mask, st);
        d_mask = mask;
    }
    VisJob J;
    memset(&J, 0, sizeof(J));
    J.bin = g;
    J.binfast = c->dev.binfast;
    J.keep = c->dev.keep;
    J.halo = p->halo;
    J.min_through = p->min_through;
    J.vote_num = p->vote_num;
    J.vote_den = p->vote_den;
    J.gap_abs = p->gap_abs;
    J.gap_rel = p->gap_rel;
    J.pts = (const float4*)d_xyzi;
    J.mask = d_mask;
    J.pairs = (const VisPair*)(blk + b_img);
    J.scans = (const VisScan*)(blk + b_img + b_pairs);
    J.tiles = (const StackTile*)(blk + b_img + b_pairs + b_scans);
    J.n_tiles = (int32_t)n_tiles;
    J.images = images;
    J.votes = o.d_votes;
    J.verdict = o.d_verdict;
    J.scan_counts = (unsigned long long*)o.d_scan_counts;
    J.counters = c->vis_counters;
    launch_vis_image(J, st);
    if (!images_only) launch_vis_vote(J, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

int scvod_visibility_device(scvod_ctx* c, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                            const int32_t* h_next_scan, const uint8_t* d_query_mask, const scvod_visibility_params* params, uint32_t* d_votes,
                            uint8_t* d_verdict, float* d_images, int64_t* d_scan_counts, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_scans < 0 || (n_scans > 0 && !h_scan_offsets)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    const VisOut o = {d_votes, d_verdict, d_images, d_scan_counts};
    if (int rc = vis_check(c, params, o)) return rc;
    if (n_scans > 0 && h_scan_offsets[0] < 0) return fail(c, SCVOD_ERR_INVALID, "scan offsets must not start below 0");
    for (int s = 0; s < n_scans; ++s)
        if (h_scan_offsets[s + 1] < h_scan_offsets[s]) return fail(c, SCVOD_ERR_INVALID, "scan offsets decrease at scan %d", s);
    std::vector<int32_t> begin, viewers;
    if (vis_viewers(h_next_scan, n_scans, params->before, params->after, begin, viewers))
        return fail(c, SCVOD_ERR_INVALID, "visibility: h_next_scan names a scan outside the batch, a scan itself, one successor twice or a ring");
    const bool any = n_scans > 0 && h_scan_offsets[n_scans] > h_scan_offsets[0];
    if (any && !d_xyzi) return fail(c, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    if ((uintptr_t)d_xyzi & 15u) return fail(c, SCVOD_ERR_INVALID, "d_xyzi is not 16-byte aligned");
    return vis_run(c, d_xyzi, h_scan_offsets, n_scans, h_poses, begin, viewers, d_query_mask, false, params, o, stream ? (hipStream_t)stream : c->stream);
}

int scvod_batch_visibility(scvod_ctx* c, const float* h_poses, const int32_t* h_next_scan, const scvod_visibility_params* params, int32_t flags,
                           uint32_t* d_votes, uint8_t* d_verdict, float* d_images, int64_t* d_scan_counts, void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    const VisOut o = {d_votes, d_verdict, d_images, d_scan_counts};
    if (int rc = vis_check(c, params, o)) return rc;
    if (flags & ~(SCVOD_VIS_WITH_GROUND | SCVOD_VIS_IMAGES_ONLY))
        return fail(c, SCVOD_ERR_INVALID, "scvod_batch_visibility: flags %d: SCVOD_VIS_WITH_GROUND and SCVOD_VIS_IMAGES_ONLY are known", flags);
    const bool images_only = (flags & SCVOD_VIS_IMAGES_ONLY) != 0;
    if (images_only && (d_votes || d_verdict || d_scan_counts)) return fail(c, SCVOD_ERR_INVALID, "SCVOD_VIS_IMAGES_ONLY writes the range images only");
    const bool all = images_only || (flags & SCVOD_VIS_WITH_GROUND) != 0;
    if (!c->batch_valid || c->batch_mode == 3 || !c->A.pts)
        return fail(c, SCVOD_ERR_STATE, "scvod_batch_visibility needs a processed batch of input clouds");
    if (!all && !c->have_patchwork) return fail(c, SCVOD_ERR_STATE, "the last batch ran without Patchwork: it has no non-ground list (SCVOD_VIS_WITH_GROUND asks every point)");
    const int B = c->A.n_scans;
    std::vector<int32_t> begin, viewers;
    if (vis_viewers(h_next_scan, B, params->before, params->after, begin, viewers))
        return fail(c, SCVOD_ERR_INVALID, "visibility: h_next_scan names a scan outside the batch, a scan itself, one successor twice or a ring");
    hipStream_t st = stream ? (hipStream_t)stream : (c->last_stream ? c->last_stream : c->stream);
    return vis_run(c, c->A.pts, c->h_scan_off.data(), B, h_poses, begin, viewers, nullptr, !all, params, o, st, images_only);
}

int scvod_visibility_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->vis.ran) return fail(c, SCVOD_ERR_STATE, "scvod_visibility_stats before the first vote");
    if (int rc = read_counters(c, c->vis_counters, 8, c->vis.stream, h_out8)) return rc;
    h_out8[6] = h_out8[2] + h_out8[3] + h_out8[4] + h_out8[5];
    h_out8[7] = 0;
    return SCVOD_OK;
}

int64_t scvod_visibility_scratch_bytes(scvod_ctx* c) { return c ? (int64_t)(c->vis.cap + (c->vis_counters ? 8 * sizeof(unsigned long long) : 0)) : 0; }

// ---- a cloud against every scan's range image (scvod_cloudvis.hip) ----
int scvod_cloud_visibility_device(scvod_ctx* c, const void* d_xyzi, int64_t n, const float* d_images, const float* h_poses, int32_t n_scans,
                                  const scvod_cloud_visibility_params* params, int32_t flags, uint16_t* d_votes, uint8_t* d_verdict,
                                  void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!params || n < 0 || n_scans < 0 || n_scans > 65535) return fail(c, SCVOD_ERR_INVALID, "bad arguments (n_scans 0..65535)");
    if (cvis_check_params(params))
        return fail(c, SCVOD_ERR_INVALID,
                    "cloud visibility: halo %d 0 or 1, vote %d / %d with 0 <= num <= 1 << 20 and 1 <= den <= 1 << 20, gaps %g + %g * dis and max_range %g finite and >= 0, reserved %d 0",
                    params->halo, params->vote_num, params->vote_den, (double)params->gap_abs, (double)params->gap_rel, (double)params->max_range,
                    params->reserved);
    if (flags & ~SCVOD_CVIS_NO_SORT) return fail(c, SCVOD_ERR_INVALID, "scvod_cloud_visibility_device: flags %d: SCVOD_CVIS_NO_SORT is known", flags);
    if (n_scans > 0 && !d_images) return fail(c, SCVOD_ERR_INVALID, "NULL images of %d scans", n_scans);
    if (n > 0 && !d_xyzi) return fail(c, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    if ((uintptr_t)d_xyzi & 15u) return fail(c, SCVOD_ERR_INVALID, "d_xyzi is not 16-byte aligned");
    if ((uintptr_t)d_images & 15u) return fail(c, SCVOD_ERR_INVALID, "d_images is not 16-byte aligned");
    if ((uintptr_t)d_votes & 7u) return fail(c, SCVOD_ERR_INVALID, "d_votes is not 8-byte aligned");
    if (n > 2147483647ll) return fail(c, SCVOD_ERR_CAPACITY, "more than 2^31 - 1 points");
    const BinParams& g = c->dev.bin;
    if (g.azimuth_num <= 0 || g.sector_num <= 0) return fail(c, SCVOD_ERR_INVALID, "the ctx's grid has no pixels");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    const bool sorted = !(flags & SCVOD_CVIS_NO_SORT) && n > 0;
    // the block: [matrices][keys in, out][indices in, out][rocprim's temporary storage]
    const size_t b_T = align_up(sizeof(float) * 12 * (size_t)n_scans, 256), b_n = sorted ? align_up(4 * (size_t)n, 256) : 0;
    const size_t b_tmp = sorted ? align_up(cvis_sort_bytes(n), 256) : 0;
    c->cv_host.assign(12 * (size_t)n_scans, 0.f);
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < n_scans; ++s) scvod_pose_delta(zero, h_poses ? h_poses + 6 * (size_t)s : zero, c->cv_host.data() + 12 * (size_t)s);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = counter_block(c, &c->cv_counters, 10)) return rc;
    if (int rc = scratch_reserve(c, c->cv, b_T + 4 * b_n + b_tmp + 256)) return rc;  // (waits for the call in flight before the block moves)
    unsigned char* blk = (unsigned char*)c->cv.buf;
    c->cv.stream = st;
    c->cv.ran = true;
    HIPCHK(c, hipMemsetAsync(c->cv_counters, 0, 10 * sizeof(unsigned long long), st));
    if (n == 0) return SCVOD_OK;
    if (n_scans > 0)
        if (int rc = staged_upload(c, c->cv_host.data(), sizeof(float) * 12 * (size_t)n_scans, blk, st)) return rc;
    const uint32_t* order = nullptr;
    if (sorted) {
        uint32_t* key_in = (uint32_t*)(blk + b_T);
        uint32_t* key_out = (uint32_t*)(blk + b_T + b_n);
        uint32_t* idx_in = (uint32_t*)(blk + b_T + 2 * b_n);
        uint32_t* idx_out = (uint32_t*)(blk + b_T + 3 * b_n);
        launch_cvis_key((const float4*)d_xyzi, n, key_in, idx_in, st);
        const hipError_t e = launch_cvis_sort(blk + b_T + 4 * b_n, b_tmp, key_in, key_out, idx_in, idx_out, n, st);
        if (e != hipSuccess) return fail(c, SCVOD_ERR_HIP, "rocprim radix sort: %s", hipGetErrorString(e));
        order = idx_out;
    }
    CvisJob J;
    memset(&J, 0, sizeof(J));
    J.V.bin = g;
    J.V.binfast = c->dev.binfast;
    J.V.keep = c->dev.keep;
    J.V.halo = params->halo;
    J.V.min_through = params->min_through;
    J.V.vote_num = params->vote_num;
    J.V.vote_den = params->vote_den;
    J.V.gap_abs = params->gap_abs;
    J.V.gap_rel = params->gap_rel;
    J.max_range = params->max_range;
    J.reach = params->max_range > 0.f && params->max_range < g.max_dis ? params->max_range : g.max_dis;
    J.pts = (const float4*)d_xyzi;
    J.n = n;
    J.order = order;
    J.T = (const float*)blk;
    J.images = d_images;
    J.n_scans = n_scans;
    J.votes = d_votes;
    J.verdict = d_verdict;
    J.counters = c->cv_counters;
    launch_cvis_vote(J, st);
    HIPCHK(c, hipGetLastError());
    return SCVOD_OK;
}

int scvod_cloud_visibility_stats(scvod_ctx* c, int64_t* h_out10) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out10) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->cv.ran) return fail(c, SCVOD_ERR_STATE, "scvod_cloud_visibility_stats before the first call");
    return read_counters(c, c->cv_counters, 10, c->cv.stream, h_out10);
}

int64_t scvod_cloud_visibility_scratch_bytes(scvod_ctx* c) { return c ? (int64_t)(c->cv.cap + (c->cv_counters ? 10 * sizeof(unsigned long long) : 0)) : 0; }

// ---- a map split by nearest-neighbour hits (scvod_split.hip) ----
void scvod_split_params_default(scvod_split_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->cell = 0.2f;
    p->max_rings = 3;
    p->base_stride = 3;
    p->query_stride = 3;
}

int scvod_map_split_device(scvod_ctx* c, const float* d_base, const uint32_t* d_base_label, int32_t n_base, const float* d_query,
                           int32_t n_query, const scvod_split_params* params, uint8_t* d_mark, int32_t* d_order, int64_t* d_seg4,
                           float* d_base_out, const uint32_t* d_payload_in, uint32_t* d_payload_out, int32_t* d_nn_idx, float* d_nn_sqdist,
                           void* stream) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_base < 0 || n_query < 0 || (n_base > 0 && !d_base) || (n_query > 0 && !d_query)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    scvod_split_params p;  // a copy: the caller's struct is the caller's again when the call returns
    if (params)
        p = *params;
    else
        scvod_split_params_default(&p);
    if ((p.base_stride != 3 && p.base_stride != 4) || (p.query_stride != 3 && p.query_stride != 4))
        return fail(c, SCVOD_ERR_INVALID, "strides %d / %d: 3 (packed xyz) or 4 (xyzi)", p.base_stride, p.query_stride);
    if ((p.base_stride == 4 && (((uintptr_t)d_base & 15) || ((uintptr_t)d_base_out & 15))) || (p.query_stride == 4 && ((uintptr_t)d_query & 15)))
        return fail(c, SCVOD_ERR_INVALID, "a cloud of 4 floats per record must be 16-byte aligned");
    if (d_payload_out && !d_payload_in) return fail(c, SCVOD_ERR_INVALID, "a payload output needs a payload input");
    if (p.n_reject_classes < 0 || p.n_reject_classes > 16) return fail(c, SCVOD_ERR_INVALID, "%d reject classes (0..16)", p.n_reject_classes);
    if (p.n_reject_classes > 0 && n_base > 0 && !d_base_label) return fail(c, SCVOD_ERR_INVALID, "a reject list needs the base labels");
    if (!(p.cell > 0.f) || !std::isfinite(p.cell)) return fail(c, SCVOD_ERR_INVALID, "cell must be positive and finite");
    if (p.max_rings < 1 || p.max_rings > 8) return fail(c, SCVOD_ERR_INVALID, "max_rings %d (1..8)", p.max_rings);
    if (d_base_out && n_base > 0) {
        const uintptr_t a0 = (uintptr_t)d_base, b0 = (uintptr_t)d_base_out, bytes = (uintptr_t)4 * (uintptr_t)p.base_stride * (uintptr_t)n_base;
        if (a0 < b0 + bytes && b0 < a0 + bytes) return fail(c, SCVOD_ERR_INVALID, "the record output overlaps the base cloud");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    if (int rc = counter_block(c, &c->sp_stats, 8)) return rc;
    const int32_t buckets = grid_buckets(n_base);
    if (int rc = scratch_reserve(c, c->sp, sp_work_bytes(buckets, n_base, n_query))) return rc;  // (the old block may still be read by a split in flight)
    SpJob J;
    memset(&J, 0, sizeof(J));
    J.base = d_base;
    J.base_label = d_base_label;
    J.query = d_query;
    J.n_base = n_base;
    J.n_query = n_query;
    J.base_stride = p.base_stride;
    J.query_stride = p.query_stride;
    J.max_rings = p.max_rings;
    J.n_reject = p.n_reject_classes;
    for (int k = 0; k < 16; ++k) J.reject[k] = p.reject_classes[k];
    J.mark = d_mark;
    J.order = d_order;
    J.seg4 = d_seg4;
    J.base_out = d_base_out;
    J.payload_in = d_payload_in;
    J.payload_out = d_payload_out;
    J.nn_idx = d_nn_idx;
    J.nn_sq = d_nn_sqdist;
    launch_map_split(J, p.cell, buckets, c->sp.buf, c->sp_stats, st);
    HIPCHK(c, hipGetLastError());
    c->sp.stream = st;
    c->sp.ran = true;
    return SCVOD_OK;
}

int scvod_map_split_stats(scvod_ctx* c, int64_t* h_out8) {
    if (!c) return SCVOD_ERR_INVALID;
    if (!h_out8) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    if (!c->sp.ran) return fail(c, SCVOD_ERR_STATE, "no scvod_map_split_device on this ctx yet");
    return read_counters(c, c->sp_stats, 8, c->sp.stream, h_out8);
}

int64_t scvod_map_split_scratch_bytes(scvod_ctx* c) {
    return c ? (int64_t)c->sp.cap + (c->sp_stats ? (int64_t)sizeof(unsigned long long) * 8 : 0) : 0;
}

int scvod_map_split(scvod_ctx* c, const float* h_base, const uint32_t* h_base_label, int32_t n_base, const float* h_query, int32_t n_query,
                    const scvod_split_params* params, uint8_t* h_mark, int32_t* h_order, int64_t* h_seg4, float* h_base_out) {
    if (!c) return SCVOD_ERR_INVALID;
    if (n_base < 0 || n_query < 0 || (n_base > 0 && !h_base) || (n_query > 0 && !h_query)) return fail(c, SCVOD_ERR_INVALID, "bad arguments");
    scvod_split_params p;
    if (params)
        p = *params;
    else
        scvod_split_params_default(&p);
    if ((p.base_stride != 3 && p.base_stride != 4) || (p.query_stride != 3 && p.query_stride != 4))
        return fail(c, SCVOD_ERR_INVALID, "strides %d / %d: 3 (packed xyz) or 4 (xyzi)", p.base_stride, p.query_stride);
    if (p.n_reject_classes > 0 && n_base > 0 && !h_base_label) return fail(c, SCVOD_ERR_INVALID, "a reject list needs the base labels");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nb = (size_t)(n_base > 0 ? n_base : 1), nq = (size_t)(n_query > 0 ? n_query : 1);
    const size_t b_bytes = 4 * (size_t)p.base_stride * nb, q_bytes = 4 * (size_t)p.query_stride * nq;
    // base | query | labels | records out | order | mark | seg4, each 256-byte aligned
    const size_t o_q = align_up(b_bytes, 256), o_lab = o_q + align_up(q_bytes, 256), o_out = o_lab + align_up(4 * nb, 256),
                 o_ord = o_out + align_up(b_bytes, 256), o_mark = o_ord + align_up(4 * nb, 256), o_seg = o_mark + align_up(nb, 256);
    unsigned char* d = nullptr;
    if (hipMalloc(&d, o_seg + 32) != hipSuccess) return fail(c, SCVOD_ERR_HIP, "scvod_map_split: no device memory for %d + %d points", n_base, n_query);
    int rc = SCVOD_OK;
    hipStream_t st = c->stream;
    if (n_base > 0 && hipMemcpyAsync(d, h_base, 4 * (size_t)p.base_stride * n_base, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: upload failed");
    if (rc == SCVOD_OK && n_query > 0 && hipMemcpyAsync(d + o_q, h_query, 4 * (size_t)p.query_stride * n_query, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: upload failed");
    if (rc == SCVOD_OK && n_base > 0 && h_base_label && hipMemcpyAsync(d + o_lab, h_base_label, 4 * (size_t)n_base, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: upload failed");
    if (rc == SCVOD_OK)
        rc = scvod_map_split_device(c, (const float*)d, h_base_label ? (const uint32_t*)(d + o_lab) : nullptr, n_base, (const float*)(d + o_q),
                                    n_query, &p, d + o_mark, (int32_t*)(d + o_ord), (int64_t*)(d + o_seg), (float*)(d + o_out), nullptr, nullptr,
                                    nullptr, nullptr, st);
    if (rc == SCVOD_OK && n_base > 0) {
        bool ok = true;
        if (h_mark) ok &= hipMemcpyAsync(h_mark, d + o_mark, (size_t)n_base, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (h_order) ok &= hipMemcpyAsync(h_order, d + o_ord, 4 * (size_t)n_base, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (h_base_out) ok &= hipMemcpyAsync(h_base_out, d + o_out, 4 * (size_t)p.base_stride * n_base, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (!ok) rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: download failed");
    }
    if (rc == SCVOD_OK && h_seg4 && hipMemcpyAsync(h_seg4, d + o_seg, 32, hipMemcpyDeviceToHost, st) != hipSuccess)
        rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: download failed");
    if (hipStreamSynchronize(st) != hipSuccess && rc == SCVOD_OK) rc = fail(c, SCVOD_ERR_HIP, "scvod_map_split: the stream failed");
    hipFree(d);
    return rc;
}

}  // extern "C"
