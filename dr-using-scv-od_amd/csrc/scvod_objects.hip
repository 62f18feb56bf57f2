// scvod_objects.hip -- the clusters of a batch as an object table on the device (gfx950): one 64-byte scvod_object per cluster that
// survived the bounding-box refine, the member points of every object grouped behind it, and per INPUT point the index of its object
// (scvod_batch_objects).
//
// Reference analogue: Frame::cluster_set after SSC::refineClusterByBoundingBox -- Cluster::name / type / state / bounding_box /
// occupy_pts / occupy_voxels (include/utility.h:142-162; ssc.cpp:377-385, 421-435, 437-467) and the box columns of the feature row
// of getDescriptorByEigenValue (ssc.cpp:723-751).  Everything it is made of is in the arena already:
//     pt_cluster / pt_type    canonical name (smallest apri index of the cluster: the cluster's first point names it) and type
//     cl_state / pt_dyn       what scvod_batch_track decided
//     apri_src, pts           the coordinates of an apri point
//     vox_pt_begin / vox_pts  the points of every voxel
// An object is an apri point i with pt_cluster[i] == i and pt_type[i] != 0, so the table is a stable compaction of those points: the
// list part is scvod_export.hip's (per-tile ballot counts, two small scan launches, in-wave ranks; no workgroup waits for another).
// Members: the key (object << 32 | apri position) of every member point, radix-sorted on the object bits alone -- the input is in
// ascending apri position and the sort is stable, so the members of an object come out in ascending apri index and the slot of a key
// IS its slot in the member list.  Reductions: one wave per object over its run of the sorted list -- box by integer min / max of
// the order-preserving float images (exact, order-independent), centre by three sequential fp32 chains in member order (the
// loads of 64 members are made by the wave, the additions by one chain), voxels by one thread per voxel of the scan (integer
// atomics: order-independent).  The output is the same bit for bit on every run.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "scvod_dev.h"

namespace scvod {
namespace {

constexpr uint32_t kObjNone = 0xffffffffu;  // upper key word of a point of no object (masked to the sorted bits it is their largest value)

__device__ __forceinline__ float obj_ord2f(uint32_t u) { return u2f((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// apri point c of the scan at `base` names an object: it is its cluster's first point and the box refine kept the cluster
__device__ __forceinline__ bool obj_is_root(const Arena& A, int base, int n_a, int c) {
    return (unsigned)c < (unsigned)n_a && A.pt_type[(size_t)base + c] != 0 && A.pt_cluster[(size_t)base + c] == c;
}

// tile blockIdx.x of scan blockIdx.y (apri indices): its objects and its member points
__global__ __launch_bounds__(256) void k_obj_count(Arena A, ObjectJob J) {
    __shared__ int wcnt[8];
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int i0 = blockIdx.x * kExpTile;
    int c_obj = 0, c_mem = 0;
    if (i0 < n) {
        int pc[8];
        uint8_t ty[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + u * 256 + (int)threadIdx.x, n - 1);
            pc[u] = A.pt_cluster[(size_t)base + i];
            ty[u] = A.pt_type[(size_t)base + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256 + (int)threadIdx.x;
            const bool mem = i < n && ty[u] != 0;
            c_mem += __popcll(__ballot(mem));
            c_obj += __popcll(__ballot(mem && pc[u] == i));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        wcnt[threadIdx.x >> 6] = c_obj;
        wcnt[4 + (threadIdx.x >> 6)] = c_mem;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int* w = wcnt + 4 * threadIdx.x;
        J.tile_cnt[2 * ((size_t)s * J.tiles_per_scan + blockIdx.x) + threadIdx.x] = w[0] + w[1] + w[2] + w[3];
    }
}

// per scan: its tiles' object counts -> exclusive prefix inside the scan; the scan's objects and members
__global__ __launch_bounds__(256) void k_obj_scan_tiles(ObjectJob J) {
    __shared__ int wsum[5];
    const int s = blockIdx.x;
    int32_t* cnt = J.tile_cnt + 2 * (size_t)s * J.tiles_per_scan;
    const bool in = (int)threadIdx.x < J.tiles_per_scan;
    const int v = in ? cnt[2 * threadIdx.x] : 0;
    const int m = in ? cnt[2 * threadIdx.x + 1] : 0;
    int total, total_m;
    const int ex = block_excl_scan<256>(v, total, wsum);
    block_excl_scan<256>(m, total_m, wsum);
    if (in) cnt[2 * threadIdx.x] = ex;
    if (threadIdx.x == 0) {
        J.scan_cnt[2 * s] = total;
        J.scan_cnt[2 * s + 1] = total_m;
    }
}

// one workgroup: the scans' totals -> the caller's offsets; the sizes and the overflow latch
__global__ __launch_bounds__(1024) void k_obj_scan_scans(int n_scans, ObjectJob J) {
    __shared__ int wsum[17];
    long long carry = 0, members = 0;
    for (int b = 0; b < n_scans; b += 1024) {
        const int i = b + (int)threadIdx.x;
        const int v = i < n_scans ? J.scan_cnt[2 * i] : 0;
        const int m = i < n_scans ? J.scan_cnt[2 * i + 1] : 0;
        int total, total_m;
        const int ex = block_excl_scan<1024>(v, total, wsum);
        block_excl_scan<1024>(m, total_m, wsum);
        if (i < n_scans) J.obj_off[i] = (int32_t)(carry + ex);
        carry += total;
        members += total_m;
    }
    if (threadIdx.x == 0) {
        J.obj_off[n_scans] = (int32_t)carry;
        if (J.begin) J.begin[carry] = (int32_t)members;  // (the end of the last object's run)
        J.stats[0] = J.out ? (carry < J.cap_obj ? carry : J.cap_obj) : 0;
        J.stats[1] = carry;
        J.stats[2] = members;
        J.stats[3] = ((J.out && carry > J.cap_obj) || (J.member_src && members > J.cap_mem)) ? 1 : 0;
    }
}

// the objects of tile blockIdx.x of scan blockIdx.y get their index in the table (per root, J.root_obj); their voxel counters are cleared
__global__ __launch_bounds__(256) void k_obj_index(Arena A, ObjectJob J) {
    __shared__ int wcnt[32];  // [round][wave] objects, then their exclusive prefix in (round, wave) order
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int i0 = blockIdx.x * kExpTile;
    if (i0 >= n) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    bool root[8];
    int rank[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        const int ic = min(i, n - 1);
        root[u] = i < n && A.pt_type[(size_t)base + ic] != 0 && A.pt_cluster[(size_t)base + ic] == i;
        const unsigned long long bal = __ballot(root[u]);
        rank[u] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[u * 4 + w] = __popcll(bal);
    }
    __syncthreads();
    if (w == 0) {
        const int v = lane < 32 ? wcnt[lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < 32) wcnt[lane] = inc - v;
    }
    __syncthreads();
    const int tile_base = J.obj_off[s] + J.tile_cnt[2 * ((size_t)s * J.tiles_per_scan + blockIdx.x)];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (!root[u]) continue;
        const int o = tile_base + wcnt[u * 4 + w] + rank[u];  // (< the apri points of the batch: inside root_obj / nvox)
        J.root_obj[(size_t)base + i0 + u * 256 + threadIdx.x] = o;
        J.nvox[o] = 0;
    }
}

// per INPUT slot of scan blockIdx.y: the sort key of the apri point that lives there (object << 32 | position), kObjNone for a point
// of no object and for the slots behind the scan's apri points; the object index scattered to the input point
__global__ __launch_bounds__(256) void k_obj_keys(Arena A, ObjectJob J) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int n_a = A.counts[s * 8 + 4];
    constexpr int U = 4;  // type -> cluster -> object is three dependent loads deep
    for (int i0 = blockIdx.x * (256 * U) + threadIdx.x; i0 < n; i0 += gridDim.x * (256 * U)) {
        int pc[U];
        uint32_t o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            pc[u] = (i < n_a && A.pt_type[(size_t)base + i] != 0) ? A.pt_cluster[(size_t)base + i] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)  // (a name that is not a listed root is followed nowhere: root_obj holds an index only there)
            o[u] = obj_is_root(A, base, n_a, pc[u]) ? (uint32_t)J.root_obj[(size_t)base + pc[u]] : kObjNone;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 256;
            if (i >= n) break;
            J.key_in[(size_t)base + i] = ((uint64_t)o[u] << 32) | (uint32_t)(base + i);
            if (J.point_object && o[u] != kObjNone) {
                const int src = A.apri_src[(size_t)base + i];
                if ((unsigned)src < (unsigned)n) J.point_object[(size_t)base + src] = (int32_t)o[u];
            }
        }
    }
}

// sorted slot p: where an object's run begins; the member list (the slot of a key is its slot in the list)
__global__ __launch_bounds__(256) void k_obj_begin(Arena A, ObjectJob J) {
    const long long total = A.total_pts;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const uint64_t k = J.key_out[p];
        const uint32_t o = (uint32_t)(k >> 32);
        if (o == kObjNone) continue;
        if (p == 0 || (uint32_t)(J.key_out[p - 1] >> 32) != o) J.begin[o] = (int32_t)p;
        if (J.member_src && p < J.cap_mem) J.member_src[p] = A.apri_src[(uint32_t)k];
    }
}

// occupy_voxels after sampleVec: per voxel of scan blockIdx.y, every DISTINCT object among its points counts it once (the points of
// a voxel normally share one cluster; an aliased voxel -- index triples outside the grid that meet in one key -- may hold several)
__global__ __launch_bounds__(256) void k_obj_voxels(Arena A, ObjectJob J) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int nv = A.counts[s * 8 + 6];
    const int n_a = A.counts[s * 8 + 4];
    const int32_t* vbeg = A.vox_pt_begin + base + s;
    const int32_t* vpts = A.vox_pts + base;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nv; v += gridDim.x * 256) {
        const int b = vbeg[v], e = min(vbeg[v + 1], n_a);
        int c0 = -1;  // the first object met: the only one of nearly every voxel, so its other points cost one comparison
        for (int j = b; j < e; ++j) {
            const int i = vpts[j];
            if ((unsigned)i >= (unsigned)n_a || A.pt_type[(size_t)base + i] == 0) continue;
            const int c = A.pt_cluster[(size_t)base + i];
            if (c == c0) continue;
            if (c0 < 0) c0 = c;
            bool seen = false;
            for (int q = b; q < j && !seen; ++q) {  // (an aliased voxel only: was this object met before?)
                const int iq = vpts[q];
                seen = (unsigned)iq < (unsigned)n_a && A.pt_type[(size_t)base + iq] != 0 && A.pt_cluster[(size_t)base + iq] == c;
            }
            if (!seen && obj_is_root(A, base, n_a, c)) atomicAdd(&J.nvox[J.root_obj[(size_t)base + c]], 1);
        }
    }
}

struct ObjPoint {
    float x, y, z;
};
__device__ __forceinline__ ObjPoint obj_load(const Arena& A, const uint64_t* key_out, int p, int e, int scan_base, int scan_n) {
    ObjPoint r = {0.f, 0.f, 0.f};
    if (p < e) {
        const uint32_t g = (uint32_t)key_out[p];
        const int src = A.apri_src[g];
        if ((unsigned)src < (unsigned)scan_n) {
            const float4 q = A.pts[(size_t)scan_base + src];
            r.x = q.x;
            r.y = q.y;
            r.z = q.z;
        }
    }
    return r;
}

// one wave per object: its run [begin[o], begin[o + 1]) of the sorted list, 64 members per round.  The next round's gather is in flight
// while this round is summed: the three chains s += x_k run in member order on values read lane by lane (v_readlane), identical on
// every lane, so the additions are those of one sequential loop over the cluster's points.
__global__ __launch_bounds__(256) void k_obj_reduce(Arena A, ObjectJob J, int n_scans) {
    const int lane = threadIdx.x & 63;
    const long long n_obj = J.stats[0];
    for (long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); o < n_obj; o += (long long)gridDim.x * 4) {
        const int b = J.begin[o], e = J.begin[o + 1];
        int lo = 0, hi = n_scans;  // the scan of object o: the last s with obj_off[s] <= o
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((long long)J.obj_off[mid] <= o) lo = mid; else hi = mid;
        }
        const int s = lo;
        const int base = A.scan_off[s];
        const int scan_n = A.scan_off[s + 1] - base;
        const uint32_t g0 = (uint32_t)J.key_out[b];  // the first member is the smallest apri index: the name
        uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
        float sx = 0.f, sy = 0.f, sz = 0.f;
        ObjPoint cur = obj_load(A, J.key_out, b + lane, e, base, scan_n);
        for (int j = b; j < e; j += 64) {
            const ObjPoint nxt = obj_load(A, J.key_out, j + 64 + lane, e, base, scan_n);
            if (j + lane < e) {
                const uint32_t kx = float_sort_key(cur.x), ky = float_sort_key(cur.y), kz = float_sort_key(cur.z);
                mn[0] = min(mn[0], kx), mn[1] = min(mn[1], ky), mn[2] = min(mn[2], kz);
                mx[0] = max(mx[0], kx), mx[1] = max(mx[1], ky), mx[2] = max(mx[2], kz);
            }
            if (e - j >= 64) {
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    sx += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.x), k));
                    sy += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.y), k));
                    sz += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.z), k));
                }
            } else {
                for (int k = 0; k < e - j; ++k) {
                    sx += __shfl(cur.x, k, 64);
                    sy += __shfl(cur.y, k, 64);
                    sz += __shfl(cur.z, k, 64);
                }
            }
            cur = nxt;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                mn[a] = min(mn[a], (uint32_t)__shfl_xor((int)mn[a], d, 64));
                mx[a] = max(mx[a], (uint32_t)__shfl_xor((int)mx[a], d, 64));
            }
        }
        if (lane == 0) {
            const int name = (int)g0 - base;
            const uint8_t ty = A.pt_type[g0];
            const float cnt = (float)(e - b);
            scvod_object r;
            r.scan = s;
            r.name = name;
            r.n_points = e - b;
            r.n_voxels = J.nvox[o];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                r.box_min[a] = obj_ord2f(mn[a]);
                r.box_max[a] = obj_ord2f(mx[a]);
            }
            r.center[0] = sx / cnt;
            r.center[1] = sy / cnt;
            r.center[2] = sz / cnt;
            // f_11(0, 8): |getPolarAngle(point_max) - getPolarAngle(point_min)| (ssc.cpp:731-733), PointAPRI::angle's expression
            r.angle_diff = fabs_f(polar_angle_deg(r.box_max[0], r.box_max[1]) - polar_angle_deg(r.box_min[0], r.box_min[1]));
            r.cls = (int8_t)J.cls[g0];
            r.state = (int8_t)((J.use_track && ty == 2) ? A.cl_state[g0] : -1);
            r.dynamic = (uint8_t)((J.use_track && A.pt_dyn[g0] == SCVOD_DYN_DYNAMIC) ? 1 : 0);
            r.reserved = 0;
            r.point_begin = b;
            J.out[o] = r;
        }
    }
}

// the eigenvalue descriptor of every object of the table (scvod_batch_object_shapes): one wave per object over the run k_obj_reduce
// read, gathered and handed round the same way.  Pass 1: the three centroid chains (pcl::compute3DCentroid; the rule of
// scvod_object::center, recomputed: the caller's table is not read).  Pass 2: every lane forms the six products of ITS member with
// the centroid, and the six covariance chains -- independent of each other, so they are issued interleaved -- add them in member
// order.  The sums are the same on every lane; lane 0 runs the 3x3 Jacobi and the double-precision features and writes the record.
// No LDS, nothing waits for another workgroup; records at or behind J.cap are not computed.
__global__ __launch_bounds__(256) void k_obj_shape(Arena A, ShapeJob J, int n_scans) {
    const int lane = threadIdx.x & 63;
    const long long n_all = J.tab_stats[1];
    const long long n_obj = n_all < J.cap ? n_all : J.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        J.stats[0] = n_obj;
        J.stats[1] = n_all;
        J.stats[3] = n_all > J.cap ? 1 : 0;
    }
    // one object per wave and no loop over objects: inside one, the compiler keeps the double constants of log / exp and the Jacobi's
    // masks live across the two passes and runs out of scalar registers (46 spilled); the grid covers min(cap, batch points) objects
    const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o < n_obj) {
        const int b = J.begin[o], e = J.begin[o + 1];
        const int g0 = (int)(uint32_t)J.key_out[b];  // the first member's slot in the batch
        int lo = 0, hi = n_scans;  // the scan of object o: the last s with scan_off[s] <= g0 (the table's offsets are the caller's, not read)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (A.scan_off[mid] <= g0) lo = mid; else hi = mid;
        }
        const int base = A.scan_off[lo];
        const int scan_n = A.scan_off[lo + 1] - base;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        ObjPoint cur = obj_load(A, J.key_out, b + lane, e, base, scan_n);
        for (int j = b; j < e; j += 64) {
            const ObjPoint nxt = obj_load(A, J.key_out, j + 64 + lane, e, base, scan_n);
            if (e - j >= 64) {
#pragma unroll
                for (int k = 0; k < 64; ++k) {
                    sx += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.x), k));
                    sy += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.y), k));
                    sz += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur.z), k));
                }
            } else {
                for (int k = 0; k < e - j; ++k) {
                    sx += __shfl(cur.x, k, 64);
                    sy += __shfl(cur.y, k, 64);
                    sz += __shfl(cur.z, k, 64);
                }
            }
            cur = nxt;
        }
        const float cnt = (float)(e - b);
        const float cx = sx / cnt, cy = sy / cnt, cz = sz / cnt;
        float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        cur = obj_load(A, J.key_out, b + lane, e, base, scan_n);
        for (int j = b; j < e; j += 64) {
            const ObjPoint nxt = obj_load(A, J.key_out, j + 64 + lane, e, base, scan_n);
            float pr[6];
            shape_products(cur.x, cur.y, cur.z, cx, cy, cz, pr);
            if (e - j >= 64) {
                for (int k0 = 0; k0 < 64; k0 += 8) {  // (eight members per trip: 48 values in scalar registers at a time, not 384)
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
#pragma unroll
                        for (int a = 0; a < 6; ++a) c6[a] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pr[a]), k0 + k));
                    }
                }
            } else {
                for (int k = 0; k < e - j; ++k) {
#pragma unroll
                    for (int a = 0; a < 6; ++a) c6[a] += __shfl(pr[a], k, 64);
                }
            }
            cur = nxt;
        }
        if (lane == 0) {
            ObjShape r;
            shape_finish(c6, e - b, J.K, r);
            J.out[o] = r;
            if (r.flags & 1) atomicAdd((unsigned long long*)&J.stats[2], 1ull);
        }
    }
}

}  // namespace

void launch_object_shapes(const Arena& A, const ShapeJob& J, hipStream_t st) {
    hipMemsetAsync(J.stats, 0, sizeof(long long) * 4, st);
    long long waves = J.cap < A.total_pts ? J.cap : A.total_pts;  // (an object has at least one of the batch's points)
    if (waves < 1) waves = 1;                                    // (block 0 writes the stats)
    hipLaunchKernelGGL(k_obj_shape, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, A, J, A.n_scans);
}

int obj_sort_bits(long long total_pts) {  // bits that hold every object index of the batch AND the masked kObjNone above them
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= total_pts) ++bits;
    return bits;
}

size_t obj_sort_bytes(long long cap_pts) {
    size_t bytes = 0;
    rocprim::radix_sort_keys(nullptr, bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)(cap_pts > 0 ? cap_pts : 1), 32, 64, (hipStream_t)0);
    return bytes;
}

hipError_t launch_objects(const Arena& A, const ObjectJob& J, void* sort_tmp, size_t sort_bytes, hipStream_t st) {
    const int tps = J.tiles_per_scan;
    const dim3 tiles(tps > 0 ? tps : 1, A.n_scans);
    if (tps > 0) hipLaunchKernelGGL(k_obj_count, tiles, dim3(256), 0, st, A, J);
    hipLaunchKernelGGL(k_obj_scan_tiles, dim3(A.n_scans), dim3(256), 0, st, J);
    hipLaunchKernelGGL(k_obj_scan_scans, dim3(1), dim3(1024), 0, st, A.n_scans, J);
    if (!J.key_in || tps <= 0 || A.total_pts <= 0) return hipSuccess;  // count only, or a batch without points
    hipLaunchKernelGGL(k_obj_index, tiles, dim3(256), 0, st, A, J);
    hipLaunchKernelGGL(k_obj_keys, dim3((A.max_scan_pts + 1023) / 1024, A.n_scans), dim3(256), 0, st, A, J);
    size_t b = sort_bytes;
    const hipError_t e = rocprim::radix_sort_keys(sort_tmp, b, J.key_in, J.key_out, (size_t)A.total_pts, 32, 32 + obj_sort_bits(A.total_pts), st);
    if (e != hipSuccess) return e;
    const long long blocks = (A.total_pts + 255) / 256;
    hipLaunchKernelGGL(k_obj_begin, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, A, J);
    if (!J.out) return hipSuccess;
    hipLaunchKernelGGL(k_obj_voxels, dim3((A.max_scan_pts + 255) / 256 < 64 ? (A.max_scan_pts + 255) / 256 : 64, A.n_scans), dim3(256), 0, st, A, J);
    hipLaunchKernelGGL(k_obj_reduce, dim3(4096), dim3(256), 0, st, A, J, A.n_scans);
    return hipSuccess;
}

}  // namespace scvod
