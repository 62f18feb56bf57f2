// ------------------------------------------------------------------------------------------
// intensity merge of the clusters: SSC::refineClusterByIntensity (ssc.cpp:571-635), opt-in (scvod_set_intensity_merge).
// One workgroup per scan, after k_cc_scan / k_cc_exact.  Per iteration the reference visits the clusters in sort1 order, collects
// the labels S of the neighbour voxels that pass the intensity tests (findVoxelNeighbors(search_c), ssc.cpp:395-411), and fuses S
// when it holds more than one label that no earlier cluster of the iteration took.  What a cluster's S can hold depends on voxels
// only, so the neighbour walk runs once:
//   pairs  -- every (cluster of a voxel, label of a qualifying neighbour) with two different labels, sorted and unique; a flag per
//             cluster for "its own label is in S".  Qualifying neighbours have cov <= intensity_cov: only those are indexed, by rows
//             (range, azimuth) of the grid whose starts sit in LDS; a row's keys are sorted by sector.
//   walk   -- one wave visits the clusters that have a pair (no other can have |S| > 1) in descending key order (DESIGN 2), with the
//             invalid set as an LDS bitmap over names.
//   apply  -- fusions are disjoint: every member points at the smallest name (nxt); pairs are mapped through it for the next iteration.
//   finish -- post-merge names per point (pt_merged), counts, boxes and types of the fused clusters (cc_type_rule, the clustering's
//             own rule) written over pt_type / cl_count.  pt_cluster keeps the pre-merge partition (the max_name pass reads it).
// ------------------------------------------------------------------------------------------
constexpr int kImThreads = 1024;

// ascending sort of a[0, n) by one workgroup (global memory).  Bitonic network in the form whose every compare puts the smaller key
// at the lower index: positions >= n act as +inf and never move, so n needs no padding.
__device__ void im_sort(uint64_t* a, int n) {
    if (n < 2) return;
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (p2 >> 1); t += kImThreads) {
                const int lo = (t / j) * 2 * j + (t % j);
                const int hi = (j == (k >> 1)) ? (lo ^ (k - 1)) : lo + j;
                if (hi < n) {
                    const uint64_t x = a[lo], y = a[hi];
                    if (y < x) {
                        a[lo] = y;
                        a[hi] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// drops repeats from the sorted a[0, n) in place; returns the new length
__device__ int im_unique(uint64_t* a, int n, int* wsum) {
    int out = 0;
    for (int i0 = 0; i0 < n; i0 += kImThreads) {
        __syncthreads();  // (the previous chunk's writes)
        const int i = i0 + threadIdx.x;
        uint64_t v = 0;
        bool keep = false;
        if (i < n) {
            v = a[i];
            keep = i == 0 || a[i - 1] != v;
        }
        int total;
        const int ex = block_excl_scan<kImThreads>(keep ? 1 : 0, total, wsum);
        if (keep) a[out + ex] = v;
        out += total;
    }
    __syncthreads();
    return out;
}

__device__ __forceinline__ bool im_bit(const uint32_t* b, int i) { return (b[i >> 5] >> (i & 31)) & 1u; }

__global__ __launch_bounds__(kImThreads) void k_im_merge(DevParams P, Arena A, MergeJob M, int from_apri) {
    extern __shared__ int im_smem[];
    __shared__ int wsum[kImThreads / 64 + 1];
    __shared__ int sh[4];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int nv = A.counts[s * 8 + 6];
    if (n <= 0) return;
    const int R = P.bin.range_num, S = P.bin.sector_num, Az = P.bin.azimuth_num, rows = R * Az;
    int* rs = im_smem;                                      // [rows + 1] first qualifying voxel of each (range, azimuth) row
    uint32_t* inv = (uint32_t*)(im_smem + rows + 1);        // [(n + 31) / 32] invalid_name of the current iteration
    const int nw = (n + 31) >> 5;
    const int32_t* vkey = A.vox_key + base;
    const int32_t* vbeg = A.vox_pt_begin + base + s;
    const int32_t* vpts = A.vox_pts + base;
    const float* vav = A.vox_av + base;
    const float* vcov = A.vox_cov + base;
    const int32_t* idx3 = A.apri_idx3 + base;
    const int32_t* ptc = A.pt_cluster + base;
    int32_t* vlab = M.vlab + base;
    int32_t* key0 = M.key0 + base;
    int32_t* nxt = M.nxt + base;
    uint8_t* own = M.own + base;
    uint8_t* fz = M.fz + base;
    int32_t* qv = M.qv + base;
    int32_t* qk = M.qk + base;
    uint32_t* box = M.box + 7 * (size_t)base;
    uint64_t* pair = M.pair + (size_t)kImPairsPerPt * base + (size_t)kImPairsPerScan * s;
    uint64_t* cand = M.cand + base;
    int32_t* merged = M.pt_merged + base;
    const int cap = kImPairsPerPt * n + kImPairsPerScan;

    int before = 0;
    for (int i0 = 0; i0 < n; i0 += kImThreads) {
        const int i = i0 + tid;
        if (i < n) {
            key0[i] = 0x7fffffff;
            nxt[i] = -1;
            own[i] = 0;
            fz[i] = 0;
        }
        before += __syncthreads_count(i < n && ptc[i] == i);  // (a cluster's name is its smallest point)
    }
    for (int v = tid; v < nv; v += kImThreads) vlab[v] = ptc[vpts[vbeg[v]]];
    int nq = 0;
    for (int v0 = 0; v0 < nv; v0 += kImThreads) {
        const int v = v0 + tid;
        const bool q = v < nv && vcov[v] <= M.cov;
        int total;
        const int ex = block_excl_scan<kImThreads>(q ? 1 : 0, total, wsum);
        if (q) {
            qv[nq + ex] = v;
            qk[nq + ex] = vkey[v];
        }
        nq += total;
    }
    if (tid == 0) sh[0] = 0;
    __syncthreads();
    for (int r = tid; r <= rows; r += kImThreads) {
        const long long k = (long long)r * S;
        int lo = 0, hi = nq;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if ((long long)qk[m] < k) lo = m + 1; else hi = m;
        }
        rs[r] = lo;
    }
    __syncthreads();

    // ---- pairs: for every voxel v and every cluster among its points (one, except for index aliasing next to the -1 bins), the
    // neighbours of the voxel's stored triple (that of its first point, makeHashCloud ssc.cpp:265-268)
    const double far = (double)R * 0.6;
    for (int v = tid; v < nv; v += kImThreads) {
        const int t = idx3[vpts[vbeg[v]]];
        const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
        const int rad = ((double)ri > far) ? 1 : M.search_c;  // ssc.cpp:397-399
        const float av = vav[v];
        const int kv = vkey[v];
        const int xlo = max(ri - rad, 0), xhi = min(ri + rad, R - 1);
        const int ylo = max(si - rad, 0), yhi = min(si + rad, S - 1);
        const int zlo = max(ai - rad, 0), zhi = min(ai + rad, Az - 1);
        int prev = -1;
        for (int k = vbeg[v]; k < vbeg[v + 1]; ++k) {
            const int c = ptc[vpts[k]];
            if (c == prev) continue;
            prev = c;
            atomicMin(&key0[c], kv);
            if (ylo > yhi) continue;
            int l0 = -1, l1 = -1, l2 = -1, l3 = -1;  // labels this item emitted last (most pairs repeat)
            for (int x = xlo; x <= xhi; ++x)
                for (int z = zlo; z <= zhi; ++z) {
                    const int row = x + z * R;
                    const long long k0 = (long long)row * S + ylo, k1 = (long long)row * S + yhi;
                    int lo = rs[row], hi = rs[row + 1];
                    while (lo < hi) {
                        const int m = (lo + hi) >> 1;
                        if ((long long)qk[m] < k0) lo = m + 1; else hi = m;
                    }
                    for (int j = lo; j < rs[row + 1] && (long long)qk[j] <= k1; ++j) {
                        const int u = qv[j];
                        if (!(fabsf(av - vav[u]) <= M.diff)) continue;  // ssc.cpp:591 (fp32)
                        const int L = vlab[u];
                        if (L == c) {
                            own[c] = 1;
                        } else if (L != l0 && L != l1 && L != l2 && L != l3) {
                            l3 = l2;
                            l2 = l1;
                            l1 = l0;
                            l0 = L;
                            const int at = atomicAdd(&sh[0], 1);
                            if (at < cap) pair[at] = ((uint64_t)(uint32_t)c << 32) | (uint32_t)L;
                        }
                    }
                }
        }
    }
    __syncthreads();
    int np = sh[0];
    const bool overflow = np > cap;
    if (overflow) np = 0;  // (counted: the scan keeps the clustering's partition)
    im_sort(pair, np);
    np = im_unique(pair, np, wsum);

    int fusions = 0, absorbed = 0;  // (wave 0)
    for (int it = 0; it < M.iterations && np > 0; ++it) {
        for (int w = tid; w < nw; w += kImThreads) inv[w] = 0u;
        // the clusters that have a pair, in descending order of their key (equal keys -- clusters that share an aliased voxel next to
        // the -1 bins -- in ascending name: the low word is the index of the cluster's first pair, and pairs are sorted by name)
        int nc = 0;
        for (int j0 = 0; j0 < np; j0 += kImThreads) {
            const int j = j0 + tid;
            const int c = j < np ? (int)(pair[j] >> 32) : -1;
            const bool first = j < np && (j == 0 || (int)(pair[j - 1] >> 32) != c);
            int total;
            const int ex = block_excl_scan<kImThreads>(first ? 1 : 0, total, wsum);
            if (first) cand[nc + ex] = ((uint64_t)(~(uint32_t)key0[c]) << 32) | (uint32_t)j;
            nc += total;
        }
        __syncthreads();
        im_sort(cand, nc);
        if (tid < 64) {
            for (int q = 0; q < nc; ++q) {
                const int j0 = (int)(uint32_t)cand[q];
                const int c = (int)(pair[j0] >> 32);
                if (im_bit(inv, c)) continue;
                const bool self = own[c] != 0;
                int cnt = self ? 1 : 0, mn = self ? c : 0x7fffffff;
                for (int jb = j0;; jb += 64) {
                    const int j = jb + lane;
                    const uint64_t p = j < np ? pair[j] : ~0ull;
                    const bool in = j < np && (int)(p >> 32) == c;
                    const int L = (int)(uint32_t)p;
                    const bool val = in && !im_bit(inv, L);
                    cnt += __popcll(__ballot(val));
                    int m = val ? L : 0x7fffffff;
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) m = min(m, __shfl_xor(m, d));
                    mn = min(mn, m);
                    if (!__shfl(in ? 1 : 0, 63)) break;
                }
                if (cnt <= 1) continue;
                for (int jb = j0;; jb += 64) {  // |S| > 1: S joins invalid_name and fuses into its smallest name
                    const int j = jb + lane;
                    const uint64_t p = j < np ? pair[j] : ~0ull;
                    const bool in = j < np && (int)(p >> 32) == c;
                    const int L = (int)(uint32_t)p;
                    if (in && !im_bit(inv, L)) {
                        atomicOr(&inv[L >> 5], 1u << (L & 31));
                        nxt[L] = mn;
                    }
                    if (!__shfl(in ? 1 : 0, 63)) break;
                }
                if (lane == 0) {
                    if (self) {
                        atomicOr(&inv[c >> 5], 1u << (c & 31));
                        nxt[c] = mn;
                    }
                    fz[mn] = 1;
                }
                ++fusions;
                absorbed += cnt - 1;
            }
        }
        __syncthreads();
        // apply: a fused cluster's S holds its own label when a member's did or when two members were neighbours
        for (int i = tid; i < n; i += kImThreads)
            if (im_bit(inv, i) && own[i]) own[nxt[i]] = 1;
        for (int j = tid; j < np; j += kImThreads) {
            const uint64_t p = pair[j];
            int c = (int)(p >> 32), L = (int)(uint32_t)p;
            if (im_bit(inv, c)) c = nxt[c];
            if (im_bit(inv, L)) L = nxt[L];
            if (c == L) {
                own[c] = 1;
                pair[j] = ~0ull;  // (sorts last, dropped below)
            } else {
                pair[j] = ((uint64_t)(uint32_t)c << 32) | (uint32_t)L;
            }
        }
        __syncthreads();
        im_sort(pair, np);
        np = im_unique(pair, np, wsum);
        if (np > 0 && pair[np - 1] == ~0ull) --np;
        __syncthreads();
    }

    // ---- finish: names, counts, boxes, types
    auto resolve = [&](int c) -> int {
        int r = c;
        for (int q = nxt[r]; q >= 0 && q != r; q = nxt[r]) r = q;
        return r;
    };
    auto fused_root = [&](int r) -> bool { return fz[r] && nxt[r] == r; };
    for (int i = tid; i < n; i += kImThreads) {
        const int r = resolve(ptc[i]);
        merged[i] = r;
        if (fused_root(r) && ptc[i] == i) {  // first visit of a fused cluster's name: its box
            uint32_t* b = box + 7 * (size_t)r;
            b[0] = b[1] = b[2] = 0xffffffffu;
            b[3] = b[4] = b[5] = 0u;
            b[6] = 0u;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kImThreads) {
        const int r = merged[i];
        if (!fused_root(r)) continue;
        uint32_t* b = box + 7 * (size_t)r;
        if (ptc[i] == i) atomicAdd(&b[6], (uint32_t)A.cl_count[(size_t)base + i]);  // occupy_pts of a member (kept at its name)
        float4 q;
        if (from_apri) {
            const scvod_apri& a = A.apri[(size_t)base + i];
            q = make_float4(a.x, a.y, a.z, 0.f);
        } else {
            q = A.pts[base + A.apri_src[(size_t)base + i]];
        }
        atomicMin(&b[0], f2ord(q.x));
        atomicMin(&b[1], f2ord(q.y));
        atomicMin(&b[2], f2ord(q.z));
        atomicMax(&b[3], f2ord(q.x));
        atomicMax(&b[4], f2ord(q.y));
        atomicMax(&b[5], f2ord(q.z));
    }
    __syncthreads();
    for (int r = tid; r < n; r += kImThreads) {
        if (!fused_root(r)) continue;
        uint32_t* b = box + 7 * (size_t)r;
        const int cnt = (int)b[6];
        const uint32_t t = cc_type_rule(P, ord2f(b[0]), ord2f(b[1]), ord2f(b[2]), ord2f(b[3]), ord2f(b[4]), ord2f(b[5]), cnt);
        A.cl_count[(size_t)base + r] = cnt;
        b[0] = t;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kImThreads) {
        const int r = merged[i];
        if (fused_root(r)) A.pt_type[(size_t)base + i] = (uint8_t)box[7 * (size_t)r];
    }
    if (tid == 0) {
        atomicAdd(&M.stats[0], before);
        atomicAdd(&M.stats[1], fusions);
        atomicAdd(&M.stats[2], before - absorbed);
        if (fusions > 0) atomicAdd(&M.stats[3], 1);
        if (overflow) atomicAdd(&M.stats[4], 1);
    }
}

// What the tracking kernels read, on the fused partition (ssc.cpp:622-627 relabels the voxels of a fused cluster): the successor
// table entries of the voxels whose first point sits in a fused cluster ({key, label, |occupy_voxels|, type}, vox_rep), and the
// car lists of the whole scan -- car clusters in ascending name, their member lists, their label ids -- as k_cc_scan writes them,
// with the per-input-point car marks of the fused clusters' points.  A scan without a fusion keeps what k_cc_scan wrote.
__global__ __launch_bounds__(kImThreads) void k_im_tables(DevParams P, Arena A, MergeJob M, int from_apri) {
    __shared__ int wsum[kImThreads / 64 + 1];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int nv = A.counts[s * 8 + 6];
    if (n <= 0) return;
    const int32_t* merged = M.pt_merged + base;
    const uint8_t* fz = M.fz + base;
    const int32_t* nxt = M.nxt + base;
    const uint8_t* ptype = A.pt_type + base;
    const int32_t* vbeg = A.vox_pt_begin + base + s;
    const int32_t* vpts = A.vox_pts + base;
    uint32_t* box = M.box + 7 * (size_t)base;  // [0] type (k_im_merge), [1] voxels, [2] lowest voxel slot
    auto fused_root = [&](int r) -> bool { return fz[r] && nxt[r] == r; };
    int any = 0;
    for (int i0 = 0; i0 < n; i0 += kImThreads) any |= __syncthreads_or(i0 + tid < n && fused_root(i0 + tid));
    if (!any) return;
    for (int r = tid; r < n; r += kImThreads)
        if (fused_root(r)) {
            box[7 * (size_t)r + 1] = 0u;
            box[7 * (size_t)r + 2] = 0x7fffffffu;
        }
    __syncthreads();
    for (int v = tid; v < nv; v += kImThreads) {
        const int r = merged[vpts[vbeg[v]]];
        if (!fused_root(r)) continue;
        atomicAdd(&box[7 * (size_t)r + 1], 1u);
        atomicMin(&box[7 * (size_t)r + 2], (uint32_t)v);
    }
    __syncthreads();
    for (int v = tid; v < nv; v += kImThreads) {
        const int r = merged[vpts[vbeg[v]]];
        if (!fused_root(r)) continue;
        const uint32_t* b = box + 7 * (size_t)r;
        const int t = (int)b[0];
        A.vox_track[(size_t)base + v] = make_int4(A.vox_key[(size_t)base + v], t ? r : -1, t ? (int)b[1] : 0, t);
        A.vox_rep[(size_t)base + v] = t ? (int)b[2] : -1;
    }
    __syncthreads();
    // car clusters: a name is the cluster's smallest point, so ascending point order is ascending name order
    int* rank_cur = M.key0 + base;  // [n] per car name: cursor of its member list (the merge's keys are used up)
    int* minslot = M.qv + base;     // [n] per car name: lowest voxel slot carrying its label (label id in the chain)
    int ncar = 0;
    for (int i0 = 0; i0 < n; i0 += kImThreads) {
        const int i = i0 + tid;
        const bool car = i < n && merged[i] == i && ptype[i] == 2;
        int total;
        const int ex = block_excl_scan<kImThreads>(car ? 1 : 0, total, wsum);
        if (car) {
            A.tk_clusters[(size_t)base + ncar + ex] = i;
            minslot[i] = 0x7fffffff;
        }
        ncar += total;
    }
    __syncthreads();
    for (int v = tid; v < nv; v += kImThreads) {
        const int lab = A.vox_track[(size_t)base + v].y;
        if (lab >= 0 && merged[lab] == lab && ptype[lab] == 2) atomicMin(&minslot[lab], v);
    }
    __syncthreads();
    int run = 0;
    for (int j0 = 0; j0 < ncar; j0 += kImThreads) {
        const int j = j0 + tid;
        const int name = j < ncar ? A.tk_clusters[(size_t)base + j] : 0;
        const int cnt = j < ncar ? A.cl_count[(size_t)base + name] : 0;
        int total;
        const int ex = block_excl_scan<kImThreads>(cnt, total, wsum);
        if (j < ncar) {
            A.tk_mbegin[(size_t)base + name] = run + ex;
            A.tk_crep[(size_t)base + j] = minslot[name];
            rank_cur[name] = 0;
        }
        run += total;
    }
    if (tid == 0) {
        A.tk_scan[s * 4 + 0] = ncar;
        A.tk_scan[s * 4 + 1] = run;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kImThreads) {
        const int r = merged[i];
        const bool car = ptype[i] == 2;
        if (car) {
            const int at = atomicAdd(&rank_cur[r], 1);
            A.tk_members[(size_t)base + A.tk_mbegin[(size_t)base + r] + at] = i;
        }
        if (!from_apri && fused_root(r)) A.pt_mapcls[(size_t)base + A.apri_src[(size_t)base + i]] = car ? kMapCar : (uint8_t)0;
    }
}

// Frame::max_name after the merge: the fused cluster that contains the carrier scvod_lastname.hip found takes the number (it holds
// the largest running number alive).  The voxel slot stays: the chain checks that its label is still the carrier's.
__global__ void k_im_lastname(Arena A, MergeJob M) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= A.n_scans) return;
    const int name = A.cc_last[(size_t)s * 4];
    if (name >= 0) A.cc_last[(size_t)s * 4] = M.pt_merged[(size_t)A.scan_off[s] + name];
}
