// CPU replay of the pad-free LDS sort schedule (dr-using-scv-od_amd/csrc/scvod_sortnet.h): every
// pass, thread by thread, through the same pass_item / run_store templates the kernels call, on an
// array that records who touches what.  Built and driven by tests/test_sortnet_host.py.
//
//   sortnet_replay full|quick <seed>
//
// prints "passes <lge> <np2> <count>" for every network met and "ok <cases>" at the end; any
// violation prints a line starting with FAIL and the exit status is 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../dr-using-scv-od_amd/csrc/scvod_sortnet.h"

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

template <typename T>
struct Lds {
    std::vector<T> data;
    std::vector<int> owner;     // thread that touched the slot since the last barrier, -1 = none
    std::vector<char> allowed;  // physical slot of a logical index < nlive
    int thread = 0;
    T poison;
    Lds(int np2, int nlive, T poison_) : poison(poison_) {
        const int slots = sortnet::slot(true, np2) + 8;
        data.assign(slots, poison);
        owner.assign(slots, -1);
        allowed.assign(slots, 0);
        for (int i = 0; i < nlive; ++i) allowed[sortnet::slot(true, i)] = 1;
    }
    void touch(int s) {
        if (s < 0 || s >= (int)data.size()) {
            FAIL("slot %d outside the array", s);
            std::exit(1);
        }
        if (!allowed[s]) FAIL("thread %d touches dead slot %d", thread, s);
        if (owner[s] != -1 && owner[s] != thread) FAIL("slot %d touched by threads %d and %d in one pass", s, owner[s], thread);
        owner[s] = thread;
    }
    void barrier() { std::fill(owner.begin(), owner.end(), -1); }
};
template <typename T>
struct Ref {
    Lds<T>* l;
    int s;
    operator T() const {
        l->touch(s);
        return l->data[s];
    }
    Ref& operator=(T v) {
        l->touch(s);
        l->data[s] = v;
        return *this;
    }
};
template <typename T>
struct Arr {
    Lds<T>* l;
    Ref<T> operator[](int s) const { return Ref<T>{l, s}; }
};
struct Cx {
    template <typename T>
    void operator()(T& lo, T& hi) const {
        if (hi < lo) std::swap(lo, hi);
    }
};

// the tier a patch of n keys is sorted in (k_pw_sort / k_vx_bucket launches): capacity, threads, start
struct Tier {
    int cap, threads, np2;
    bool from_regs;
};
static Tier tier_of(int n, int lge) {
    static const int caps[] = {256, 1024, 2048, 4096, 8192, 16384};
    int cap = 16384;
    for (int c : caps)
        if (n < c) {
            cap = c;
            break;
        }
    Tier t;
    t.cap = cap;
    t.threads = std::max(64, cap >> lge);
    t.np2 = 1 << lge;
    while (t.np2 < n) t.np2 <<= 1;
    t.from_regs = cap >= 4096 && t.np2 == cap && (cap / t.threads) == (1 << lge);
    return t;
}

static std::map<std::pair<int, int>, int> g_passes;

template <int LGE, typename T>
static void replay(int n, const std::vector<T>& keys, T padv, T poison) {
    constexpr int E = 1 << LGE;
    const Tier tr = tier_of(n, LGE);
    const int np2 = tr.np2, TH = tr.threads;
    const int nlive = sortnet::live_end(n, LGE);
    if (nlive % E || nlive < n || nlive - n >= E || nlive > np2) FAIL("live_end(%d, %d) = %d", n, LGE, nlive);
    Lds<T> lds(np2, nlive, poison);
    Arr<T> a{&lds};
    if (tr.from_regs) {
        std::vector<char> seen(n, 0);
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            if (t >= (nlive >> LGE)) continue;
            T e[E];
            for (int it = 0; it < E; ++it) {
                const int j = sortnet::start_key(it, t, nlive, LGE);
                if (j < n) {
                    if (seen[j]) FAIL("key %d loaded twice", j);
                    seen[j] = 1;
                }
                e[it] = (j < n) ? keys[j] : padv;
            }
            sortnet::run_store<LGE, true>(e, a, t, Cx{});
        }
        for (int j = 0; j < n; ++j)
            if (!seen[j]) FAIL("key %d never loaded (n %d)", j, n);
    } else {
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            for (int j = t; j < nlive; j += TH) a[sortnet::slot(true, j)] = (j < n) ? keys[j] : padv;
        }
        lds.barrier();
        for (int t = 0; t < TH; ++t) {
            lds.thread = t;
            for (int g = t; g < (nlive >> LGE); g += TH) {
                T e[E];
                for (int m = 0; m < E; ++m) e[m] = a[sortnet::slot(true, (g << LGE) + m)];
                sortnet::run_store<LGE, true>(e, a, g, Cx{});
            }
        }
    }
    lds.barrier();
    int passes = 0;
    sortnet::for_each_pass<LGE>(np2, [&](int r, int lt, bool mirror) {
        ++passes;
        const int items = sortnet::pass_items(np2, nlive, r, lt);
        // every item left out must be dead
        for (int t = items; t < (np2 >> lt); ++t)
            if (sortnet::item_base(t, r, lt) < nlive) FAIL("pass r=%d lt=%d drops live item %d (n %d)", r, lt, t, n);
        for (int th = 0; th < TH; ++th) {
            lds.thread = th;
            for (int t = th; t < items; t += TH) {
                if (!mirror)
                    sortnet::pass_item<LGE, false, true, T>(a, t, r, nlive, padv, Cx{});
                else if (lt == 1)
                    sortnet::pass_item<1, true, true, T>(a, t, r, nlive, padv, Cx{});
                else if (lt == 2)
                    sortnet::pass_item<2, true, true, T>(a, t, r, nlive, padv, Cx{});
                else if (lt == 3)
                    sortnet::pass_item<3, true, true, T>(a, t, r, nlive, padv, Cx{});
                else
                    sortnet::pass_item<4, true, true, T>(a, t, r, nlive, padv, Cx{});
            }
        }
        lds.barrier();
    });
    int lg = 0;
    while ((1 << lg) < np2) ++lg;
    if (passes != sortnet::merge_passes(lg, LGE)) FAIL("merge_passes(%d, %d) != %d", lg, LGE, passes);
    auto it = g_passes.find({LGE, np2});
    if (it == g_passes.end())
        g_passes[{LGE, np2}] = passes;
    else if (it->second != passes)
        FAIL("pass count of np2 %d depends on n", np2);
    std::vector<T> want(keys.begin(), keys.begin() + n);
    std::sort(want.begin(), want.end());
    for (int j = 0; j < nlive; ++j) {
        const T got = lds.data[sortnet::slot(true, j)];
        const T w = (j < n) ? want[j] : padv;
        if (got != w) {
            FAIL("n %d lge %d: slot %d holds %llx, want %llx", n, LGE, j, (unsigned long long)got, (unsigned long long)w);
            break;
        }
    }
    for (size_t s = 0; s < lds.data.size(); ++s)
        if (!lds.allowed[s] && lds.data[s] != poison) FAIL("n %d lge %d: dead slot %zu written", n, LGE, s);
}

static long g_cases = 0;
static void run_n(int n, std::mt19937_64& rng) {
    // unique 64-bit keys in the kernels' form (exponent | z << 19 | index), with many z ties; pad 2.0
    std::vector<uint64_t> k64(n);
    std::vector<uint32_t> k32(n);
    const uint32_t zr = 1u + (uint32_t)(rng() % 400);
    for (int j = 0; j < n; ++j) {
        k64[j] = (0x3ffull << 52) | ((uint64_t)(rng() % zr) << 19) | (uint64_t)j;
        k32[j] = (uint32_t)(rng() % (zr * 3));  // repeats
    }
    std::shuffle(k64.begin(), k64.end(), rng);
    replay<3, uint64_t>(n, k64, 0x4000000000000000ull, 0xdeadbeefdeadbeefull);
    replay<4, uint64_t>(n, k64, 0x4000000000000000ull, 0xdeadbeefdeadbeefull);
    replay<3, uint32_t>(n, k32, 0xffffffffu, 0xdeadbeefu);
    replay<4, uint32_t>(n, k32, 0xffffffffu, 0xdeadbeefu);
    g_cases += 4;
}

int main(int argc, char** argv) {
    const bool full = argc > 1 && !std::strcmp(argv[1], "full");
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);
    std::set<int> ns;
    for (int n = 1; n <= (full ? 1100 : 140); ++n) ns.insert(n);
    for (int np2 : {2048, 4096, 8192, 16384}) {
        auto add = [&](int n) {
            if (n >= 1 && n <= 16384) ns.insert(n);
        };
        const int w = full ? 17 : 1;
        for (int c : {np2 / 2, 3 * np2 / 4, np2})
            for (int d = -w; d <= w; ++d) add(c + d);
        // multiples of the thread counts of the tier (16 and 8 keys per thread), a seeded sample
        for (int th : {np2 >> 4, np2 >> 3})
            for (int i = 0; i < (full ? 6 : 1); ++i) {
                const int mult = th * (int)(np2 / 2 / th + 1 + rng() % (np2 / 2 / th));
                for (int d = -1; d <= 1; ++d) add(mult + d);
            }
        for (int i = 0; i < (full ? 200 : 3); ++i) add(np2 / 2 + 1 + (int)(rng() % (np2 / 2)));
    }
    for (int n : ns) run_n(n, rng);
    for (auto& p : g_passes) std::printf("passes %d %d %d\n", p.first.first, p.first.second, p.second);
    if (g_fail) {
        std::printf("FAILED %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok %ld\n", g_cases);
    return 0;
}
