"""numpy statements the static-map tests share (tests/test_pose_matrix.py, tests/test_gpu_map_table.py): the record packing and the
table hash of csrc/scvod_map.hip restated, the fp32 definition of a point's record, the fp64 decode of a record and the fp64 pose
from elementary rotations.  Nothing here calls the library."""
import numpy as np

CELL_BITS = 21
CELL_BIAS = 1 << 20
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)   # key of an empty slot / of a padding record
MAX_PROBES = 512                      # kMapMaxProbes
_U = np.uint64


def map_mix(k):
    """murmur3 finaliser on uint64 -- MUST follow map_mix of scvod_map.hip (the tests pick keys by their home slot with it)"""
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> _U(33)
        k *= _U(0xFF51AFD7ED558CCD)
        k ^= k >> _U(33)
        k *= _U(0xC4CEB9FE1A85EC53)
        k ^= k >> _U(33)
    return k


def home(k, capacity):
    return (map_mix(k) & _U(capacity - 1)).astype(np.int64)


def pack_key(cx, cy, cz):
    u = [(np.asarray(c, np.int64) + CELL_BIAS).astype(np.uint64) for c in (cx, cy, cz)]
    return (u[0] << _U(2 * CELL_BITS)) | (u[1] << _U(CELL_BITS)) | u[2]


def unpack_key(key):
    key = np.asarray(key, np.uint64)
    m = _U((1 << CELL_BITS) - 1)
    return [((key >> _U(s)) & m).astype(np.int64) - CELL_BIAS for s in (2 * CELL_BITS, CELL_BITS, 0)]


def pack_val(qx, qy, qz, qi):
    q = [np.asarray(v, np.int64).astype(np.uint64) for v in (qx, qy, qz, qi)]
    return (q[0] << _U(48)) | (q[1] << _U(32)) | (q[2] << _U(16)) | q[3]


def unpack_val(val):
    val = np.asarray(val, np.uint64)
    return [((val >> _U(s)) & _U(0xFFFF)).astype(np.int64) for s in (48, 32, 16, 0)]


def random_keys(rng, n):
    """n distinct valid keys (63 bits, so never the padding key)"""
    k = np.unique(rng.integers(0, 1 << 63, size=2 * n + 16, dtype=np.uint64))
    assert len(k) >= n
    return rng.permutation(k)[:n]


def reduce_records(keys, vals):
    """the definition of a merge: per distinct key the smallest value, padding ignored, sorted by key"""
    keys, vals = np.asarray(keys, np.uint64).ravel(), np.asarray(vals, np.uint64).ravel()
    live = keys != PAD
    keys, vals = keys[live], vals[live]
    o = np.lexsort((vals, keys))
    keys, vals = keys[o], vals[o]
    first = np.ones(len(keys), bool)
    first[1:] = keys[1:] != keys[:-1]
    return keys[first], vals[first]


def simulate_table(keys, capacity):
    """occupied slots of a linear-probing table of `capacity` slots that holds the distinct `keys` (the set does not depend on the
    insertion order), with an unbounded number of probes; needs len(keys) <= capacity"""
    keys = np.unique(np.asarray(keys, np.uint64))
    assert len(keys) <= capacity
    occ = bytearray(capacity)
    for h in home(keys, capacity).tolist():
        while occ[h]:
            h = (h + 1) & (capacity - 1)
        occ[h] = 1
    return np.frombuffer(occ, np.uint8).astype(bool)


def longest_run(occ):
    """(length of the longest circular run of occupied slots, does that run cross the end of the table)"""
    n = len(occ)
    if occ.all():
        return n, True
    start = int(np.flatnonzero(~occ)[0]) + 1            # rotate so that the sequence starts right behind an empty slot
    r = np.roll(occ, -start)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], r.astype(np.int8), [0]])))
    if len(edges) == 0:
        return 0, False
    b, e = edges[0::2], edges[1::2]
    i = int(np.argmax(e - b))
    first, last = (int(b[i]) + start) % n, (int(e[i]) - 1 + start) % n
    return int(e[i] - b[i]), last < first


def sorted_records(m):
    rec = m.export().cpu().numpy().view(np.uint64).reshape(-1, 2)
    o = np.argsort(rec[:, 0])
    return rec[o, 0], rec[o, 1]


def to_device(keys, vals):
    import torch
    rec = np.stack([np.asarray(keys, np.uint64), np.asarray(vals, np.uint64)], axis=1).view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(rec)).cuda()


def decode_points(keys, vals, leaf):
    """fp64 statement of scvod_map_points: (cell + (offset + 0.5) / 65536) * leaf per axis (leaf = the map's fp32 edge), and the
    intensity (val & 0xffff) / 256"""
    c, q = unpack_key(keys), unpack_val(vals)
    lf = np.float64(np.float32(leaf))
    xyz = np.stack([(c[i].astype(np.float64) + (q[i].astype(np.float64) + 0.5) / 65536.0) * lf for i in range(3)], axis=1)
    return xyz, q[3].astype(np.float64) / 256.0


def encode_points(T, p, leaf):
    """fp32 definition of k_map_accumulate + map_encode for the points p [n, 4] of one scan under the row-major 3x4 matrix T:
    (keys, vals, in_range).  Products and sums are rounded one by one, in the order the kernel writes them."""
    T, p = np.asarray(T, np.float32), np.asarray(p, np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(over="ignore", invalid="ignore"):
        w = [((T[4 * i] * p[:, 0] + T[4 * i + 1] * p[:, 1]) + T[4 * i + 2] * p[:, 2]) + T[4 * i + 3] for i in range(3)]
        f = [c * inv for c in w]
        c = [np.floor(v) for v in f]
        ok = np.ones(len(p), bool)
        for ci in c:
            ok &= (ci >= -float(CELL_BIAS)) & (ci < float(CELL_BIAS))
        ci = [np.where(ok, v, 0).astype(np.int64) for v in c]
        q = [np.clip(np.where(ok, (fi - cc) * np.float32(65536.0), 0).astype(np.int64), 0, 65535) for fi, cc in zip(f, c)]
        qi = np.clip(p[:, 3] * np.float32(256.0), np.float32(0), np.float32(65535)).astype(np.int64)
    return pack_key(*ci), pack_val(q[0], q[1], q[2], qi), ok


def rot64(roll, pitch, yaw):
    """R = Rz(yaw) @ Ry(pitch) @ Rx(roll) in fp64 from the three elementary rotations (what pcl::getTransformation means)"""
    r, p, y = np.float64(roll), np.float64(pitch), np.float64(yaw)
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], np.float64)
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], np.float64)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


def pose64(pose):
    """4x4 fp64 matrix of a pose (x, y, z, roll, pitch, yaw) given in fp32"""
    p = np.asarray(pose, np.float32).astype(np.float64)
    M = np.eye(4)
    M[:3, :3] = rot64(p[3], p[4], p[5])
    M[:3, 3] = p[:3]
    return M


def poses64(poses):
    """the same for poses [n, 6] at once: [n, 4, 4]"""
    p = np.asarray(poses, np.float32).astype(np.float64).reshape(-1, 6)
    n = len(p)
    cr, sr, cp, sp, cy, sy = np.cos(p[:, 3]), np.sin(p[:, 3]), np.cos(p[:, 4]), np.sin(p[:, 4]), np.cos(p[:, 5]), np.sin(p[:, 5])
    z, o = np.zeros(n), np.ones(n)
    Rx = np.stack([o, z, z, z, cr, -sr, z, sr, cr], axis=1).reshape(n, 3, 3)
    Ry = np.stack([cp, z, sp, z, o, z, -sp, z, cp], axis=1).reshape(n, 3, 3)
    Rz = np.stack([cy, -sy, z, sy, cy, z, z, z, o], axis=1).reshape(n, 3, 3)
    M = np.tile(np.eye(4), (n, 1, 1))
    M[:, :3, :3] = Rz @ Ry @ Rx
    M[:, :3, 3] = p[:, :3]
    return M
