// CPU replay of the box-grid kNN search (dr-using-scv-od_amd/csrc/scvod_boxgrid.h): the shape rule, the cell rule,
// the ring walk, the top-k insertion and the stop rule are the header's own functions; only the CSR table is
// filled serially here (the header's build needs a workgroup), in the header's convention (cell[id] = end of id).
// Built and driven by tests/test_boxgrid_host.py.
//
//   boxgrid_replay full|quick <seed>
//
// prints "ok <checks>" at the end; any violation prints a line starting with FAIL and the exit status is 1.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../dr-using-scv-od_amd/csrc/scvod_boxgrid.h"

using namespace scvod;

static int g_fail = 0;
static long g_checks = 0;
#define FAIL(...)                      \
    do {                               \
        if (g_fail < 20) {             \
            std::printf("FAIL ");      \
            std::printf(__VA_ARGS__);  \
            std::printf("\n");         \
        }                              \
        ++g_fail;                      \
    } while (0)

// ---- 1. the rings of a query cell partition the grid, and the bound turns infinite exactly when they have
static void ring_partition(int dx, int dy, int dz) {
    const BoxGrid g{0.f, 0.f, 0.f, 1.f, dx, dy, dz};
    const int nc = dx * dy * dz;
    std::vector<int> seen(nc);
    for (int cz = 0; cz < dz; ++cz)
        for (int cy = 0; cy < dy; ++cy)
            for (int cx = 0; cx < dx; ++cx) {
                std::fill(seen.begin(), seen.end(), 0);
                const int R = std::max({cx, dx - 1 - cx, cy, dy - 1 - cy, cz, dz - 1 - cz});  // the ring that completes the grid
                const float qx = cx + 0.5f, qy = cy + 0.5f, qz = cz + 0.5f;
                if (bg_cell(g, qx, qy, qz) != bg_cell_id(g, cx, cy, cz)) FAIL("cell of the centre of (%d %d %d)", cx, cy, cz);
                for (int r = 0; r <= R; ++r) {
                    bg_ring_runs(g, cx, cy, cz, r, [&](int ia, int ib, int oz, int oy) {
                        if (ia < 0 || ib >= nc || ia > ib) {
                            FAIL("grid %dx%dx%d cell (%d %d %d) ring %d: run [%d, %d]", dx, dy, dz, cx, cy, cz, r, ia, ib);
                            return;
                        }
                        if (ia / dx != ib / dx || ia / dx != (cz + oz) * dy + (cy + oy)) FAIL("ring %d: run [%d, %d] is not in row (%d, %d)", r, ia, ib, oz, oy);
                        for (int id = ia; id <= ib; ++id) {
                            const int x = id % dx, y = (id / dx) % dy, z = id / (dx * dy);
                            const int cheb = std::max({std::abs(x - cx), std::abs(y - cy), std::abs(z - cz)});
                            if (cheb != r) FAIL("ring %d hands out cell %d at distance %d", r, id, cheb);
                            ++seen[id];
                        }
                    });
                    const bool whole = bg_unprobed(g, cx, cy, cz, r, qx, qy, qz) == INFINITY;
                    if (whole != (r == R)) FAIL("grid %dx%dx%d cell (%d %d %d): whole-grid report %d at ring %d, complete at %d", dx, dy, dz, cx, cy, cz, (int)whole, r, R);
                    if (whole && !bg_stop(INFINITY, bg_margin(g), INFINITY)) FAIL("bg_stop goes on past the whole grid");
                }
                for (int id = 0; id < nc; ++id)
                    if (seen[id] != 1) {
                        FAIL("grid %dx%dx%d cell (%d %d %d): cell %d visited %d times", dx, dy, dz, cx, cy, cz, id, seen[id]);
                        break;
                    }
                ++g_checks;
            }
}

// ---- 2. the shape rule against the two blocks it replaced, transcribed
struct Shape {
    float h;
    int dx, dy, dz;
};
static Shape shape_region_growing(float ex, float ey, float ez, int n) {
    float a = fmaxf(ex, fmaxf(ey, ez)), cmin = fminf(ex, fminf(ey, ez));
    const float b = ex + ey + ez - a - cmin;
    float h = fmaxf(fmaxf(sqrtf(a * b / (float)n) * 1.5f, cbrtf(a * b * cmin / (float)n)), 2.f * a / (float)n);
    if (!(h > 0.f)) h = 1.f;
    int dx, dy, dz;
    for (;;) {
        dx = (int)fminf(ex / h, 1.0e6f) + 1;
        dy = (int)fminf(ey / h, 1.0e6f) + 1;
        dz = (int)fminf(ez / h, 1.0e6f) + 1;
        if ((double)dx * dy * dz <= 2.0 * n) break;
        h *= 1.25f;
    }
    return Shape{h, dx, dy, dz};
}
static Shape shape_calibration(float ex, float ey, float ez, int n) {
    const float a = fmaxf(ex, fmaxf(ey, ez)), cmin = fminf(ex, fminf(ey, ez));
    const float b = ex + ey + ez - a - cmin;
    float h = fmaxf(fmaxf(sqrtf(a * b / (float)n) * 0.5f, cbrtf(a * b * cmin / (float)n) * 0.5f), 2.f * a / (float)n);
    if (!(h > 0.f) || !(h < 3.0e38f)) h = 1.f;
    int dx, dy, dz;
    for (;;) {
        dx = (int)fminf(ex / h, 1.0e6f) + 1;
        dy = (int)fminf(ey / h, 1.0e6f) + 1;
        dz = (int)fminf(ez / h, 1.0e6f) + 1;
        if ((double)dx * dy * dz <= 2.0 * n) break;
        h *= 1.125f;
    }
    return Shape{h, dx, dy, dz};
}
// (first_stage 1: an extent whose products overflow, which only the calibration's whole scans are guarded against)
static void shape_check(const char* what, float ex, float ey, float ez, int n, int first_stage = 0) {
    for (int stage = first_stage; stage < 2; ++stage) {
        const Shape w = stage ? shape_calibration(ex, ey, ez, n) : shape_region_growing(ex, ey, ez, n);
        const BoxGrid g = bg_shape(1.f, 2.f, 3.f, ex, ey, ez, n, stage ? kCalShape : kRgShape);
        if (f2u(g.h) != f2u(w.h) || g.dx != w.dx || g.dy != w.dy || g.dz != w.dz)
            FAIL("%s stage %d: shape %08x %d %d %d, the transcription gives %08x %d %d %d", what, stage, f2u(g.h), g.dx, g.dy, g.dz, f2u(w.h), w.dx, w.dy, w.dz);
        if ((double)g.dx * g.dy * g.dz > 2.0 * n || g.dx < 1 || g.dy < 1 || g.dz < 1) FAIL("%s stage %d: %d x %d x %d cells for %d points", what, stage, g.dx, g.dy, g.dz, n);
        ++g_checks;
    }
}

// ---- 3. the search against brute force
struct Cloud {
    std::string name;
    std::vector<float> x, y, z;
    int n() const { return (int)x.size(); }
    void add(float a, float b, float c) {
        x.push_back(a);
        y.push_back(b);
        z.push_back(c);
    }
};

static void search_check(const Cloud& c, const BoxShape shape, int stage, int k, int stride) {
    const int n = c.n();
    float mn[3] = {c.x[0], c.y[0], c.z[0]}, mx[3] = {c.x[0], c.y[0], c.z[0]};
    for (int i = 0; i < n; ++i) {
        const float p[3] = {c.x[i], c.y[i], c.z[i]};
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], p[a]);
            mx[a] = std::max(mx[a], p[a]);
        }
    }
    shape_check(c.name.c_str(), mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], n);
    const BoxGrid g = bg_shape(mn[0], mn[1], mn[2], mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2], n, shape);
    const int nc = g.dx * g.dy * g.dz;
    std::vector<int> cell(nc + 1, 0), pcell(n), order(n);
    for (int i = 0; i < n; ++i) {
        pcell[i] = bg_cell(g, c.x[i], c.y[i], c.z[i]);
        if (pcell[i] < 0 || pcell[i] >= nc) {
            FAIL("%s: point %d in cell %d of %d", c.name.c_str(), i, pcell[i], nc);
            return;
        }
        ++cell[pcell[i]];
    }
    for (int id = 0, run = 0; id <= nc; ++id) {  // exclusive scan, then the cursor scatter: cell[id] ends as the END of id
        const int v = cell[id];
        cell[id] = run;
        run += v;
    }
    for (int i = n - 1; i >= 0; --i) order[cell[pcell[i]]++] = i;  // (any order inside a cell: here the reversed one)
    const int keff = std::min(n, k);
    const float mg = bg_margin(g);
    const int rmax = std::max({g.dx, g.dy, g.dz});
    std::vector<std::pair<float, int>> all(n);
    for (int p = 0; p < n; p += stride) {
        const float qx = c.x[p], qy = c.y[p], qz = c.z[p];
        const int cx = bg_cell1(qx, g.ox, g.h, g.dx), cy = bg_cell1(qy, g.oy, g.h, g.dy), cz = bg_cell1(qz, g.oz, g.h, g.dz);
        float bd[kBoxGridK], kth;
        int bq[kBoxGridK], kq;
        bg_topk_clear(bd, bq, kth, kq);
        int r = 0;
        for (;; ++r) {
            if (r > rmax) {
                FAIL("%s: query %d does not stop", c.name.c_str(), p);
                return;
            }
            bg_ring_runs(g, cx, cy, cz, r, [&](int ia, int ib, int, int) {
                int b, e;
                bg_run(cell.data(), ia, ib, b, e);
                for (int t = b; t < e; ++t) {
                    const int q = order[t];
                    bg_topk_insert(bg_dist2(c.x[q], c.y[q], c.z[q], qx, qy, qz), q, keff, bd, bq, kth, kq);
                }
            });
            if (bg_stop(bg_unprobed(g, cx, cy, cz, r, qx, qy, qz), mg, kth)) break;
        }
        for (int q = 0; q < n; ++q) {
            const float ddx = c.x[q] - qx, ddy = c.y[q] - qy, ddz = c.z[q] - qz;
            all[q] = {(ddx * ddx + ddy * ddy) + ddz * ddz, q};
        }
        std::partial_sort(all.begin(), all.begin() + keff, all.end());
        for (int j = 0; j < kBoxGridK; ++j) {
            const bool held = j < keff;
            const float wd = held ? all[j].first : INFINITY;
            const int wq = held ? all[j].second : 0x7fffffff;
            if (f2u(bd[j]) != f2u(wd) || bq[j] != wq) {
                FAIL("%s stage %d k %d query %d entry %d: (%a, %d), brute force (%a, %d); stopped at ring %d of %dx%dx%d", c.name.c_str(), stage, k, p, j, bd[j], bq[j], wd,
                     wq, r, g.dx, g.dy, g.dz);
                break;
            }
        }
        if (f2u(kth) != f2u(bd[keff - 1]) || kq != bq[keff - 1]) FAIL("%s: the k-th mirror differs from entry %d", c.name.c_str(), keff - 1);
        ++g_checks;
    }
}

static std::vector<Cloud> clouds(std::mt19937_64& rng, bool full) {
    auto uni = [&](float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 40) * (1.0 / 16777216.0)); };
    std::vector<Cloud> v;
    {
        Cloud c{"one point"};
        c.add(3.5f, -2.25f, 0.75f);
        v.push_back(c);
    }
    {
        Cloud c{"two points"};
        c.add(3.5f, -2.25f, 0.75f);
        c.add(3.75f, -2.f, 1.f);
        v.push_back(c);
    }
    {
        Cloud c{"seven points"};
        for (int i = 0; i < 7; ++i) c.add(uni(10.f, 11.f), uni(-4.f, -3.f), uni(0.f, 2.f));
        v.push_back(c);
    }
    {
        Cloud c{"500 copies"};
        for (int i = 0; i < 500; ++i) c.add(12.125f, 7.5f, -1.0625f);
        v.push_back(c);
    }
    {
        Cloud c{"tie lattice"};  // every coordinate and every d^2 exact: rows of equal distances
        const int m = full ? 9 : 6;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j)
                for (int l = 0; l < m; ++l) c.add(20.f + 0.25f * i, -8.f + 0.25f * j, 0.25f * l);
        v.push_back(c);
    }
    {
        Cloud c{"plane"};
        for (int i = 0; i < (full ? 1500 : 300); ++i) c.add(uni(5.f, 9.f), uni(-3.f, 3.f), 1.5f);
        v.push_back(c);
    }
    {
        Cloud c{"line"};
        for (int i = 0; i < 300; ++i) c.add(uni(-30.f, 30.f), 4.f, -1.f);
        v.push_back(c);
    }
    {
        Cloud c{"scan around +-80 m"};  // a dense near field, a sparse far field
        for (int i = 0; i < (full ? 2000 : 300); ++i) c.add(uni(-6.f, 6.f), uni(-6.f, 6.f), uni(-1.5f, 1.f));
        for (int i = 0; i < (full ? 1000 : 150); ++i) c.add(uni(-80.f, 80.f), uni(-80.f, 80.f), uni(-3.f, 5.f));
        v.push_back(c);
    }
    {
        Cloud c{"wall at -80 m"};  // a cluster far from the origin: the margin's |origin| term
        for (int i = 0; i < (full ? 1200 : 250); ++i) c.add(-80.f + uni(0.f, 0.05f), uni(-79.f, -73.f), uni(-1.f, 3.f));
        v.push_back(c);
    }
    {
        Cloud c{"blob at +80 m"};
        for (int i = 0; i < (full ? 900 : 200); ++i) c.add(uni(79.f, 81.f), uni(78.f, 80.5f), uni(0.f, 1.5f));
        v.push_back(c);
    }
    return v;
}

int main(int argc, char** argv) {
    const bool full = argc > 1 && !std::strcmp(argv[1], "full");
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
    std::mt19937_64 rng(seed);

    const int fixed[][3] = {{1, 1, 1}, {1, 5, 7}, {6, 1, 4}, {5, 3, 1}, {1, 1, 9}, {1, 8, 1}, {12, 1, 1}, {2, 2, 2}, {3, 4, 5}};
    for (auto& f : fixed) ring_partition(f[0], f[1], f[2]);
    const int top = full ? 12 : 5;
    for (int i = 0; i < (full ? 36 : 6); ++i) ring_partition(1 + (int)(rng() % top), 1 + (int)(rng() % top), 1 + (int)(rng() % top));

    // boxes no cloud below has: zero, tiny, huge and (the last two) overflowing extents
    const float ext[][3] = {{0.f, 0.f, 0.f}, {1e-30f, 0.f, 0.f}, {1e-20f, 1e-20f, 1e-20f}, {3.f, 0.f, 2.f}, {160.f, 160.f, 8.f}, {1e12f, 1e12f, 1e12f}, {1e19f, 1e19f, 1e19f}, {3e38f, 1.f, 1.f}};
    for (int i = 0; i < 8; ++i)
        for (int n : {1, 2, 17, 4096, 120000}) shape_check("box", ext[i][0], ext[i][1], ext[i][2], n, i >= 6 ? 1 : 0);

    for (const Cloud& c : clouds(rng, full))
        for (int stage = 0; stage < 2; ++stage)
            for (int k : {3, 10, 16}) search_check(c, stage ? kCalShape : kRgShape, stage, k, full ? 1 : 3);

    if (g_fail) {
        std::printf("FAILED %d checks\n", g_fail);
        return 1;
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
