// map_split_main.cpp -- the reference's two map tools on scvod_map_split (upload, the device stage, download):
//   src/erasor_dynamic.cpp: the points of an original map that no point of a remover's static map has as its nearest neighbour, and
//   the evaluation block of SSC::segDF (ssc.cpp:1511-1540): the original points that are hit and whose label is not rejected.
//   usage: scvod_map_split <original.pcd> <static.pcd> <out_prefix> [--reject 252[,...] --static-out FILE] [--cell C] [--max-rings R]
// writes <out_prefix>dynamic_cloud.pcd (the MISS segment, original order); with --reject the intensity field of the original map is
// read as the label (static_cast<uint32_t>(intensity), as segDF does) and FILE gets the HIT segment (evaluate_static).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/scvod.h"
#include "utility.h"

static int usage() {
    std::fprintf(stderr,
                 "usage: scvod_map_split <original.pcd> <static.pcd> <out_prefix> [--reject 252[,...] --static-out FILE] [--cell C] "
                 "[--max-rings R]\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 4) return usage();
    scvod_split_params sp;
    scvod_split_params_default(&sp);
    sp.base_stride = sp.query_stride = 4;
    std::string static_out;
    for (int a = 4; a < argc; a += 2) {
        if (a + 1 >= argc) return usage();
        const std::string k = argv[a], v = argv[a + 1];
        if (k == "--reject") {
            sp.n_reject_classes = 0;
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = std::min(v.find(',', at), v.size());
                char* end = nullptr;
                const std::string tok = v.substr(at, comma - at);
                const long cls = std::strtol(tok.c_str(), &end, 10);
                if (tok.empty() || *end || cls < 0 || cls > 0xFFFF || sp.n_reject_classes >= 16) return usage();
                sp.reject_classes[sp.n_reject_classes++] = (uint16_t)cls;
                at = comma + 1;
            }
        } else if (k == "--static-out") {
            static_out = v;
        } else if (k == "--cell") {
            sp.cell = (float)std::atof(v.c_str());
        } else if (k == "--max-rings") {
            sp.max_rings = std::atoi(v.c_str());
        } else {
            return usage();
        }
    }
    pcl::PointCloud<pcl::PointXYZI> ori, stat;
    if (!Utility::readPcd(argv[1], ori)) {
        std::fprintf(stderr, "%s load error\n", argv[1]);
        return 1;
    }
    if (!Utility::readPcd(argv[2], stat)) {
        std::fprintf(stderr, "%s load error\n", argv[2]);
        return 1;
    }
    static_assert(sizeof(pcl::PointXYZI) == 16, "a record is x y z intensity");
    const size_t n = ori.points.size(), nq = stat.points.size();
    if (n > 0x7fffffffu || nq > 0x7fffffffu) {
        std::fprintf(stderr, "too many points\n");
        return 1;
    }
    std::vector<uint32_t> label(n);
    for (size_t i = 0; i < n; ++i) label[i] = static_cast<uint32_t>(ori.points[i].intensity);
    scvod_params P;
    scvod_params_default(&P);
    scvod_ctx* ctx = nullptr;
    int rc = scvod_create(&P, nullptr, 0, 16, 1, &ctx);
    if (rc != SCVOD_OK) {
        std::fprintf(stderr, "scvod_create failed (status %d): the split is GPU-only\n", rc);
        return 1;
    }
    pcl::PointCloud<pcl::PointXYZI> out;
    out.points.resize(n);
    int64_t seg[4] = {0, 0, 0, 0};
    rc = scvod_map_split(ctx, n ? &ori.points[0].x : nullptr, sp.n_reject_classes ? label.data() : nullptr, (int32_t)n,
                         nq ? &stat.points[0].x : nullptr, (int32_t)nq, &sp, nullptr, nullptr, seg, n ? &out.points[0].x : nullptr);
    if (rc != SCVOD_OK) {
        std::fprintf(stderr, "scvod_map_split: %s (status %d)\n", scvod_last_error(ctx), rc);
        scvod_destroy(ctx);
        return 1;
    }
    scvod_destroy(ctx);
    pcl::PointCloud<pcl::PointXYZI> part;
    part.points.assign(out.points.begin() + seg[1], out.points.begin() + seg[2]);
    const std::string name = std::string(argv[3]) + "dynamic_cloud.pcd";
    if (!Utility::writePcdAscii(name, part)) {
        std::fprintf(stderr, "%s save error\n", name.c_str());
        return 1;
    }
    if (!static_out.empty()) {
        part.points.assign(out.points.begin() + seg[0], out.points.begin() + seg[1]);
        if (!Utility::writePcdAscii(static_out, part)) {
            std::fprintf(stderr, "%s save error\n", static_out.c_str());
            return 1;
        }
    }
    std::cout << "done: " << seg[1] << " hit, " << seg[2] - seg[1] << " missed, " << seg[3] - seg[2] << " gated" << std::endl;
    return 0;
}
