"""Two numpy restatements of SSC::refineClusterByIntensity (src/ssc.cpp:571-635) over one scan's voxel table.

`literal` follows the reference line by line on its running cluster numbers: sort1 (descending `occupy_voxels` vectors), the
invalid list, the fusion map, a fused cluster named after its largest member with the members' voxel lists concatenated in
ascending running-number order.  `convention` is the rule the device runs on canonical names: a cluster's sort
key is the smallest voxel key of the ORIGINAL cluster whose name (smallest apri index) it carries, a fused cluster takes the smallest
name of its members.  Both take a voxel's label from its first point and its index triple from its first point (makeHashCloud).

Voxel tables are dicts like oracle.voxelize returns: vox_key, vox_pt_begin, vox_pts, vox_av, vox_cov, idx3 (unclamped).
"""
import numpy as np


def find_voxel_neighbors(r, s, a, size, R, S, Az):
    """findVoxelNeighbors (ssc.cpp:395-411): clipped grid, no sector wrap, radius 1 beyond 0.6 R"""
    if r > R * 0.6:
        size = 1
    out = []
    for x in range(r - size, r + size + 1):
        if x > R - 1 or x < 0:
            continue
        for y in range(s - size, s + size + 1):
            if y > S - 1 or y < 0:
                continue
            for z in range(a - size, a + size + 1):
                if z > Az - 1 or z < 0:
                    continue
                out.append(x * S + y + z * R * S)
    return out


def _tables(vox, labels, grid):
    R, S, Az = grid
    key = np.asarray(vox["vox_key"], np.int64)
    beg = np.asarray(vox["vox_pt_begin"])
    pts = np.asarray(vox["vox_pts"])
    av = np.asarray(vox["vox_av"], np.float32)
    cov = np.asarray(vox["vox_cov"], np.float32)
    idx3 = np.asarray(vox["idx3"])
    nv = len(key)
    slot = {int(k): v for v, k in enumerate(key)}
    vlab = np.array([labels[pts[beg[v]]] for v in range(nv)], np.int64)
    members = {}   # cluster -> voxels of its points
    for v in range(nv):
        for p in pts[beg[v]:beg[v + 1]]:
            members.setdefault(int(labels[p]), set()).add(v)
    return key, av, cov, idx3, slot, vlab, members, (R, S, Az)


def _neighbour_set(v, key, av, cov, idx3, slot, grid, search_c, diff, cov_max):
    """the voxels n that ssc.cpp:588-594 keeps for voxel v"""
    R, S, Az = grid
    out = []
    for k in find_voxel_neighbors(int(idx3[v][0]), int(idx3[v][1]), int(idx3[v][2]), search_c, R, S, Az):
        u = slot.get(k)
        if u is None:
            continue
        if cov[u] <= np.float32(cov_max) and abs(np.float32(av[v] - av[u])) <= np.float32(diff):
            out.append(u)
    return out


def literal(vox, running, grid, iterations, search_c, diff, cov_max):
    """running: the reference's running cluster number of every apri point.  Returns the fused running number per point."""
    key, av, cov, idx3, slot, vlab, members, grid = _tables(vox, running, grid)
    occ = {c: sorted({int(key[v]) for v in vs}) for c, vs in members.items()}   # sampleVec(occupy_voxels)
    vox_of_key = {int(key[v]): v for v in range(len(key))}
    label = {int(key[v]): int(vlab[v]) for v in range(len(key))}
    owner = {c: c for c in occ}        # original running number -> current cluster
    nb = {}
    for it in range(iterations):
        clusters = sorted(occ.items(), key=lambda kv: kv[1], reverse=True)      # sort1
        invalid = []
        fusion = {}
        for c, vlist in clusters:
            if c in invalid:
                continue
            nvox = []
            for k in vlist:
                v = vox_of_key[k]
                if v not in nb:
                    nb[v] = _neighbour_set(v, key, av, cov, idx3, slot, grid, search_c, diff, cov_max)
                nvox.extend(int(key[u]) for u in nb[v])
            nvox = sorted(set(nvox))
            names = sorted({label[k] for k in nvox if label[k] not in invalid})
            if len(names) > 1:
                invalid = sorted(set(invalid) | set(names))
                fusion[c] = names
        for _, names in fusion.items():
            fused = names[-1]
            vl = []
            for f in names:
                vl.extend(occ.pop(f))
            for k in vl:
                label[k] = fused
            occ[fused] = vl
            for o, cur in owner.items():
                if cur in names:
                    owner[o] = fused
    return np.array([owner[int(c)] for c in running], np.int64)


def convention(vox, names, grid, iterations, search_c, diff, cov_max, stats=None, ties=None):
    """names: canonical cluster name (smallest apri index) per apri point.  Returns the fused canonical name per point.
    ties: how clusters with EQUAL smallest voxel keys are visited (they occur: a voxel next to the -1 bins holds points of several
    clusters) -- None: as the stable sort finds them (first voxel, then point order), "asc" / "desc": by name.  The device takes
    them in ascending name.  stats also receives fusions_per_iteration and key_ties: the number of clusters whose smallest key equals
    another's, counted over ALL clusters.  The order can matter only between tied clusters that both have a neighbour of another
    label and are visited, so key_ties > 0 says that a scan holds ties, not that one decided anything: the comparison of the three
    orders (tests/test_intensity_merge_cases.py) is the check that carries the weight."""
    key, av, cov, idx3, slot, vlab, members, grid = _tables(vox, names, grid)
    key0 = {c: min(int(key[v]) for v in vs) for c, vs in members.items()}
    vox_of = {c: set(vs) for c, vs in members.items()}
    label = vlab.copy()
    owner = {c: c for c in vox_of}
    nb = {}
    n_before = len(vox_of)
    n_fusions = 0
    per_iteration = []
    order = {None: lambda c: -key0[c], "asc": lambda c: (-key0[c], c), "desc": lambda c: (-key0[c], -c)}[ties]
    for it in range(iterations):
        invalid = set()
        fusions = []
        for c in sorted(vox_of, key=order):
            if c in invalid:
                continue
            S_ = set()
            for v in vox_of[c]:
                if v not in nb:
                    nb[v] = _neighbour_set(v, key, av, cov, idx3, slot, grid, search_c, diff, cov_max)
                S_.update(int(label[u]) for u in nb[v])
            S_ -= invalid
            if len(S_) > 1:
                invalid |= S_
                fusions.append(S_)
        for S_ in fusions:
            t = min(S_)
            vs = set()
            for f in S_:
                vs |= vox_of.pop(f)
            vox_of[t] = vs
            for o, cur in owner.items():
                if cur in S_:
                    owner[o] = t
        label = np.array([owner[int(c)] for c in vlab], np.int64)   # a voxel's label: the cluster of its first point
        n_fusions += len(fusions)
        per_iteration.append(len(fusions))
    if stats is not None:
        k0 = sorted(key0.values())
        stats.update(clusters_before=n_before, fusions=n_fusions, clusters_after=len(vox_of), fusions_per_iteration=per_iteration,
                     key_ties=sum(1 for i, k in enumerate(k0) if (i and k0[i - 1] == k) or (i + 1 < len(k0) and k0[i + 1] == k)))
    return np.array([owner[int(c)] for c in names], np.int64)


def canonical(labels):
    """renames every cluster after its smallest point index"""
    labels = np.asarray(labels)
    first = {}
    for i, c in enumerate(labels):
        first.setdefault(int(c), i)
    return np.array([first[int(c)] for c in labels], np.int64)
