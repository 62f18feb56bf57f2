// CPU replay of the merge-path sort schedule of the large Patchwork tiers
// (dr-using-scv-od_amd/csrc/scvod_mergepath.h on top of scvod_sortnet.h): the register runs, the network
// stages up to the hand-over run length R and every merge level, thread by thread and barrier by barrier,
// through the same templates the kernel calls, on an array that records who touches what.  Built and driven by
// tests/test_mergepath_host.py; tests/devtools/merge_sort_count.py uses the count mode.
//
//   mergepath_replay test <seed>          the sizes, run lengths and key patterns of the test
//   mergepath_replay count <seed> n...    per n: comparisons and LDS accesses of the network and of merge at every R
//
// test prints "levels <R> <n> <count>" per sort and "ok <cases>" at the end; any violation prints a line
// starting with FAIL and the exit status is 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../dr-using-scv-od_amd/csrc/scvod_mergepath.h"

static int g_fail = 0;
#define FAIL(...)                      \
    do {                               \
        if (g_fail < 20) {             \
            std::printf("FAIL ");      \
            std::printf(__VA_ARGS__);  \
            std::printf("\n");         \
        }                              \
        ++g_fail;                      \
    } while (0)

constexpr int LGE = 4, E = 1 << LGE;
static long g_cmp = 0, g_acc = 0;

// a key that counts its comparisons
struct Key {
    uint64_t v;
    bool operator<(const Key& o) const {
        ++g_cmp;
        return v < o.v;
    }
};
constexpr uint64_t kPad = 0x4000000000000000ull, kPoison = 0xdeadbeefdeadbeefull, kSent = ~0ull;

enum Phase { NETWORK, READ, WRITE };
struct Lds {
    std::vector<Key> data;
    std::vector<int> owner;     // thread that touched (NETWORK) or wrote (WRITE) the slot since the last barrier
    std::vector<char> allowed;  // physical slot of a logical index < nlive; everything else is a guard word
    int thread = 0;
    Phase phase = NETWORK;
    Lds(int np2, int nlive) {
        const int slots = sortnet::slot(true, np2) + 8;
        data.assign(slots, Key{kPoison});
        owner.assign(slots, -1);
        allowed.assign(slots, 0);
        for (int i = 0; i < nlive; ++i) allowed[sortnet::slot(true, i)] = 1;
    }
    void touch(int s, bool write) {
        ++g_acc;
        if (s < 0 || s >= (int)data.size()) {
            FAIL("slot %d outside the array", s);
            std::exit(1);
        }
        if (!allowed[s]) FAIL("thread %d %s guard slot %d", thread, write ? "writes" : "reads", s);
        if (phase == READ) {
            if (write) FAIL("thread %d writes slot %d before the barrier of a merge level", thread, s);
            return;  // many threads may read one slot
        }
        if (phase == WRITE && !write) FAIL("thread %d reads slot %d between the barriers of a merge level's store", thread, s);
        if (owner[s] != -1 && owner[s] != thread) FAIL("slot %d touched by threads %d and %d between two barriers", s, owner[s], thread);
        owner[s] = thread;
    }
    void barrier(Phase next) {
        std::fill(owner.begin(), owner.end(), -1);
        phase = next;
    }
};
struct Ref {
    Lds* l;
    int s;
    operator Key() const {
        l->touch(s, false);
        return l->data[s];
    }
    Ref& operator=(Key v) {
        l->touch(s, true);
        l->data[s] = v;
        return *this;
    }
};
struct Arr {
    Lds* l;
    Ref operator[](int s) const { return Ref{l, s}; }
};
struct Cx {
    void operator()(Key& lo, Key& hi) const {
        if (hi < lo) std::swap(lo, hi);
    }
};

// the tier a patch of n keys is sorted in (k_pw_sort launches, 16 keys per thread): capacity, threads, start
struct Tier {
    int cap, threads, np2;
    bool from_regs;
};
static Tier tier_of(int n) {
    static const int caps[] = {256, 1024, 2048, 4096, 8192, 16384};
    int cap = 16384;
    for (int c : caps)
        if (n < c) {
            cap = c;
            break;
        }
    Tier t;
    t.cap = cap;
    t.threads = std::max(64, cap >> LGE);
    t.np2 = E;
    while (t.np2 < n) t.np2 <<= 1;
    t.from_regs = cap >= 4096 && t.np2 == cap;
    return t;
}

// R >= np2: the whole sort by the network.  Returns the number of merge levels.
static int replay(int n, const std::vector<uint64_t>& keys, int R, bool check) {
    const Tier tr = tier_of(n);
    const int np2 = tr.np2, TH = tr.threads;
    const int nlive = sortnet::live_end(n, LGE);
    if ((TH << LGE) < nlive) FAIL("n %d: %d threads do not cover %d live slots", n, TH, nlive);
    Lds lds(np2, nlive);
    Arr a{&lds};
    const Key padv{kPad};
    if (tr.from_regs) {
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            if (t >= (nlive >> LGE)) continue;
            Key e[E];
            for (int it = 0; it < E; ++it) {
                const int j = sortnet::start_key(it, t, nlive, LGE);
                e[it] = (j < n) ? Key{keys[j]} : padv;
            }
            sortnet::run_store<LGE, true>(e, a, t, Cx{});
        }
    } else {
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            for (int j = t; j < nlive; j += TH) a[sortnet::slot(true, j)] = (j < n) ? Key{keys[j]} : padv;
        }
        lds.barrier(NETWORK);
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            for (int g = t; g < (nlive >> LGE); g += TH) {
                Key e[E];
                for (int m = 0; m < E; ++m) e[m] = a[sortnet::slot(true, (g << LGE) + m)];
                sortnet::run_store<LGE, true>(e, a, g, Cx{});
            }
        }
    }
    lds.barrier(NETWORK);
    // the network's stages up to runs of R (mergepath_levels in scvod_kernels.hip)
    if (R > E) {
        sortnet::for_each_pass<LGE>(std::min(np2, R), [&](int r, int lt, bool mirror) {
            const int items = sortnet::pass_items(np2, nlive, r, lt);
            for (int th = 0; th < TH; ++th) {
                lds.thread = th;
                for (int t = th; t < items; t += TH) {
                    if (!mirror)
                        sortnet::pass_item<LGE, false, true, Key>(a, t, r, nlive, padv, Cx{});
                    else if (lt == 1)
                        sortnet::pass_item<1, true, true, Key>(a, t, r, nlive, padv, Cx{});
                    else if (lt == 2)
                        sortnet::pass_item<2, true, true, Key>(a, t, r, nlive, padv, Cx{});
                    else if (lt == 3)
                        sortnet::pass_item<3, true, true, Key>(a, t, r, nlive, padv, Cx{});
                    else
                        sortnet::pass_item<4, true, true, Key>(a, t, r, nlive, padv, Cx{});
                }
            }
            lds.barrier(NETWORK);
        });
    }
    int levels = 0;
    std::vector<Key> outs((size_t)TH * E);
    std::vector<char> mine(TH);
    std::vector<int> ia(TH);
    for (int L = R; L < nlive; L <<= 1, ++levels) {
        lds.barrier(READ);
        std::vector<Key> before;
        if (check) before = lds.data;
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            Key out[E];
            const long acc0 = g_acc;
            mine[t] = mergepath::merge_window<LGE, true, Key>(a, t, L, nlive, out, Key{kSent}, &ia[t]);
            if (!mine[t] && g_acc != acc0) FAIL("n %d L %d: idle thread %d touched the array", n, L, t);
            std::copy(out, out + E, outs.begin() + (size_t)t * E);
        }
        if (check) {
            // the windows tile [0, nlive): every live position is in the window of an active thread or in a last run without a
            // partner, and inside a pair the inputs a window consumes start where its predecessor's end
            const long cmp0 = g_cmp, acc0 = g_acc;
            for (int t = 0; t < TH; ++t) {
                const int p = t << LGE;
                if (p >= nlive) {
                    if (mine[t]) FAIL("n %d L %d: thread %d beyond the live prefix is active", n, L, t);
                    continue;
                }
                mergepath::Pair q = mergepath::pair_of(p, L, nlive);
                if (q.a0 % (2 * L) || q.a1 - q.a0 > L || q.b1 - q.b0 > L || q.b1 > nlive || q.d < 0 || q.d + E > (q.a1 - q.a0) + (q.b1 - q.b0))
                    FAIL("n %d L %d thread %d: pair [%d,%d) [%d,%d) d %d", n, L, t, q.a0, q.a1, q.b0, q.b1, q.d);
                if (q.b0 == q.b1) {
                    if (mine[t]) FAIL("n %d L %d: thread %d merges a run without a partner", n, L, t);
                    continue;
                }
                if (!mine[t]) {
                    FAIL("n %d L %d: live window of thread %d is not merged", n, L, t);
                    continue;
                }
                const int total = (q.a1 - q.a0) + (q.b1 - q.b0);
                int ie;  // where the window ends in the lower run: the next thread's split, or the end of the pair
                if (q.d + E == total) {
                    ie = q.a1 - q.a0;
                } else {
                    if (!mine[t + 1]) FAIL("n %d L %d: thread %d follows thread %d in a pair and is idle", n, L, t + 1, t);
                    ie = ia[t + 1];
                }
                if (q.d == 0 && ia[t] != 0) FAIL("n %d L %d: first window of a pair starts at %d", n, L, ia[t]);
                const int je = q.d + E - ie, jb = q.d - ia[t];
                if (ie < ia[t] || je < jb || ie > q.a1 - q.a0 || je > q.b1 - q.b0) {
                    FAIL("n %d L %d thread %d: split (%d, %d) then (%d, %d)", n, L, t, ia[t], jb, ie, je);
                    continue;
                }
                std::vector<uint64_t> want;
                for (int i = ia[t]; i < ie; ++i) want.push_back(before[sortnet::slot(true, q.a0 + i)].v);
                for (int j = jb; j < je; ++j) want.push_back(before[sortnet::slot(true, q.b0 + j)].v);
                std::sort(want.begin(), want.end());
                for (int m = 0; m < E; ++m)
                    if (outs[(size_t)t * E + m].v != want[m]) {
                        FAIL("n %d L %d thread %d: output %d is not the merge of its input ranges", n, L, t, m);
                        break;
                    }
            }
            g_cmp = cmp0;
            g_acc = acc0;
        }
        lds.barrier(WRITE);
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            if (!mine[t]) continue;
            Key out[E];
            std::copy(outs.begin() + (size_t)t * E, outs.begin() + (size_t)(t + 1) * E, out);
            mergepath::store_window<LGE, true, Key>(a, t, out);
        }
    }
    lds.barrier(NETWORK);
    if (levels != mergepath::levels(R, nlive)) FAIL("n %d R %d: %d levels, levels() says %d", n, R, levels, mergepath::levels(R, nlive));
    if (check) {
        std::vector<uint64_t> want(keys.begin(), keys.begin() + n);
        std::sort(want.begin(), want.end());
        for (int j = 0; j < nlive; ++j) {
            const uint64_t got = lds.data[sortnet::slot(true, j)].v;
            const uint64_t w = (j < n) ? want[j] : kPad;
            if (got != w) {
                FAIL("n %d R %d: slot %d holds %llx, want %llx", n, R, j, (unsigned long long)got, (unsigned long long)w);
                break;
            }
        }
        for (size_t s = 0; s < lds.data.size(); ++s)
            if (!lds.allowed[s] && lds.data[s].v != kPoison) FAIL("n %d R %d: guard slot %zu written", n, R, s);
    }
    return levels;
}

// unique keys in the kernels' form: exponent | z << 19 | index
static uint64_t key_of(uint32_t z, uint32_t idx) { return (0x3ffull << 52) | ((uint64_t)z << 19) | idx; }

static const char* kPatterns[] = {"ascending", "descending", "all z equal", "two z interleaved", "runs already merged", "random"};
static std::vector<uint64_t> make_keys(int n, int pattern, std::mt19937_64& rng) {
    std::vector<uint64_t> k(n);
    switch (pattern) {
        case 0:
            for (int j = 0; j < n; ++j) k[j] = key_of(j, j);
            break;
        case 1:
            for (int j = 0; j < n; ++j) k[j] = key_of(n - 1 - j, j);
            break;
        case 2:  // the index alone decides; indices in a shuffled order
            for (int j = 0; j < n; ++j) k[j] = key_of(77, j);
            std::shuffle(k.begin(), k.end(), rng);
            break;
        case 3:
            for (int j = 0; j < n; ++j) k[j] = key_of(j & 1, j);
            break;
        case 4:  // sorted blocks of 512 keys, the blocks in descending order
            for (int j = 0; j < n; ++j) k[j] = key_of((n / 512 - j / 512) * 512 + j % 512, j);
            break;
        default: {
            const uint32_t zr = 1u + (uint32_t)(rng() % 400);  // many z ties
            for (int j = 0; j < n; ++j) k[j] = key_of((uint32_t)(rng() % zr), j);
            std::shuffle(k.begin(), k.end(), rng);
        }
    }
    return k;
}

int main(int argc, char** argv) {
    const bool count = argc > 1 && !std::strcmp(argv[1], "count");
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    if (count) {
        // per n: "count <n> <R> <comparisons> <LDS accesses>"; R = 0 is the whole sort by the network
        for (int i = 3; i < argc; ++i) {
            const int n = std::atoi(argv[i]);
            if (n < 1 || n > 16384) continue;
            const std::vector<uint64_t> k = make_keys(n, 5, rng);
            for (int R : {0, 16, 32, 64, 128, 256, 512, 1024}) {
                g_cmp = g_acc = 0;
                replay(n, k, R ? R : 1 << 20, false);
                std::printf("count %d %d %ld %ld\n", n, R, g_cmp, g_acc);
            }
        }
        return g_fail ? 1 : 0;
    }
    long cases = 0;
    for (int n : {1, 15, 16, 17, 31, 33, 255, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192})
        for (int R : {16, 64, 256})
            for (int pat = 0; pat < 6; ++pat) {
                const int before = g_fail;
                const int lv = replay(n, make_keys(n, pat, rng), R, true);
                if (g_fail != before) std::printf("FAIL in n %d R %d pattern %s\n", n, R, kPatterns[pat]);
                if (pat == 0) std::printf("levels %d %d %d\n", R, n, lv);
                ++cases;
            }
    if (g_fail) {
        std::printf("FAILED %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
