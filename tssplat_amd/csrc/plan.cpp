// Host-side construction of the tiling plan.  build_plan is a driver: it calls the planner's stages in order -- the mesh
// (face adjacency, connected components = tet-spheres), the tiling (bisection into LDS-sized tiles with a one-ring face halo,
// re-cut into compact cells by partition.cpp), the layout (per-tile vertex lists, offsets, the staging / finish lists for
// vertices that more than one tile touches) and the tile fill (per-tile local indexing and planes).  The stages live in
// plan_mesh.cpp, plan_tiling.cpp, plan_layout.cpp and plan_planes.cpp; planner.h declares what they hand to each other.
//
// Replaces the role of libpgo in the reference's constructor
// (/root/reference/tssplat_ext/tet_spheres/tet_spheres.cpp:140-159): there the
// rest mesh becomes two global COO matrices, here it becomes per-tile planes
// of Dm^-1 (double -> fp32, as tet_spheres.cpp:43-45 rounds the matrix values)
// plus 16-bit local vertex / neighbour indices.  Pure C++17, no HIP.
#include "plan.h"

#include "planner.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

namespace tsamd {
namespace {

// TSAMD_PLAN_TIMING=1 prints the wall time of every stage of build_plan to stderr (tuning aid)
struct StageTimer {
    bool on = std::getenv("TSAMD_PLAN_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[plan] %-28s %8.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
};

int check_mesh_arguments(const float *rest, int64_t n, const int32_t *tets, int64_t m, std::string &err)
{
    if (n < 0 || m < 0 || (n > 0 && !rest) || (m > 0 && !tets)) {
        err = "null pointer or negative size";
        return ERR_INVALID;
    }
    if (n >= (int64_t(1) << 31) / 3 || m >= (int64_t(1) << 29)) {
        err = "mesh too large for 32-bit indexing";
        return ERR_INVALID;
    }
    for (int64_t i = 0; i < 4 * m; ++i)
        if (tets[i] < 0 || tets[i] >= n) {
            err = "tet index out of range at flat position " + std::to_string(i);
            return ERR_INVALID;
        }
    return OK;
}

// options -> limits: the thread count, the lane layout and what a tile may hold
int tiler_limits(const PlanOptions &opt, bool has_operator, TilerLimits &tl, std::string &err)
{
    // Default: all cores up to 32.  More did not help where it was measured (256-core EPYC 9575F host of the MI355X box, 21 M
    // tets): 32 threads 2.8 s, 64 threads 3.4 s, 128 asked (= 64) 3.4 s -- the bisection and pass A get slower, pass B (planes,
    // colouring, incidence matching: 1.0-1.1 s) does not get faster.  An explicit num_threads is honoured up to 64.
    tl.nthreads = opt.num_threads > 0 ? std::min(opt.num_threads, 64) : std::min(int(std::thread::hardware_concurrency()), 32);
    tl.nthreads = std::max(1, tl.nthreads);
    tl.spt = opt.slots_per_lane > 0 ? opt.slots_per_lane : kSlotsPerLane;
    if (tl.spt < 2 || tl.spt > 4) {
        err = "slots_per_lane must be 2, 3 or 4";
        return ERR_INVALID;
    }
    // Defaults: 768 threads x 2 slots and 80 KiB, two workgroups per CU -- with or without an explicit operator (its nine
    // extra planes live in registers, not in LDS, and the kernel still fits 80 VGPRs).  (Which block sizes go with which
    // lane layout is the launcher's business: capi.cpp.)
    if (opt.max_threads > 1024) {
        err = "max_threads exceeds 1024";
        return ERR_INVALID;
    }
    tl.max_threads = opt.max_threads > 0 ? opt.max_threads : kTileThreads;
    tl.max_threads = std::max(64, (tl.max_threads / 64) * 64);
    Limits &lim = tl.lim;
    lim.budget = opt.lds_budget > 0 ? opt.lds_budget : 80 * 1024;
    lim.pad_unit = tl.spt == 3 ? 12 : 4;
    lim.max_spad = int64_t(tl.spt) * int64_t(tl.max_threads) / lim.pad_unit * lim.pad_unit;
    lim.rebuild = opt.rebuild_dminv != 0 && !has_operator;
    if (lim.budget < tile_lds_bytes(12, 8, lim.rebuild)) {
        err = "lds_budget_bytes too small";
        return ERR_INVALID;
    }
    // LDS: 48 B per slot + 16 B per vertex at ~0.27 vertices per slot
    tl.s_cap = std::min<int64_t>(lim.max_spad, (lim.budget - kRowTabBytes - 256) / (lim.rebuild ? 58 : 53));
    tl.auto_target = opt.target_owned <= 0;
    tl.target = std::max<int64_t>(1, tl.auto_target ? int64_t(0.70 * double(tl.s_cap)) : int64_t(opt.target_owned));
    return OK;
}

}  // namespace

int build_plan(const float *rest, int64_t n, const int32_t *tets, int64_t m, const PlanOptions &opt, Plan &P,
               std::string &err, const ElementOperatorCSR *op)
{
    StageTimer timer;
    int rc = check_mesh_arguments(rest, n, tets, m, err);
    if (rc) return rc;
    timer.lap("index check");
    TilerLimits tl;
    if ((rc = tiler_limits(opt, op != nullptr, tl, err))) return rc;

    P = Plan();
    P.n = n;
    P.m = m;
    P.spt = tl.spt;
    if ((rc = build_adjacency(tets, n, m, P.nbr, tl.nthreads, err))) return rc;
    const Mesh M{rest, tets, P.nbr.data(), n, m};
    timer.lap("face adjacency");

    if (op) {
        bool symmetric = false;
        if ((rc = operator_face_weights(*op, P.nbr.data(), m, opt.rebuild_dminv != 0, P.op_diag, P.op_w, symmetric, err))) return rc;
        P.n_planes = symmetric ? kPlanesWeightedSym : kPlanesWeighted;
    }
    if (tl.lim.rebuild) P.n_planes = kPlanesRebuild;

    Components comps = connected_components(P.nbr.data(), m, tl.nthreads);
    timer.lap("components");
    P.n_components = comps.count();

    const std::vector<float> cen = tet_centroids(M, tl.nthreads);
    Workers W(tl.nthreads, m, n);
    Tiling tiling;
    group_components(M, comps, tl.lim, W, tiling);
    timer.lap("centroids + fit check");
    if ((rc = bisect_groups(M, comps, cen, tl, W, tiling, err))) return rc;
    timer.lap("bisection");
    refine_with_cells(M, comps, cen, tl, W, tiling);
    P.n_cut_components = tiling.n_cut;
    P.n_bisection_components = tiling.n_cut - tiling.n_refined;
    P.n_cut_templates = tiling.n_templates;
    if (timer.on)
        std::fprintf(stderr, "[plan] partition: %lld cut components, %lld refined, %lld keep the bisection (%lld cut themselves)\n",
                     (long long)tiling.n_cut, (long long)tiling.n_refined, (long long)(tiling.n_cut - tiling.n_refined), (long long)tiling.n_templates);
    timer.lap("partition (cells + refinement)");
    std::vector<std::vector<int32_t>> tiles_owned;
    for (auto &gt : tiling.leaves)
        for (auto &t : gt) tiles_owned.push_back(std::move(t));
    tiling = Tiling();

    const TileLists lists = list_tile_vertices(M, std::move(tiles_owned), W);
    timer.lap("pass A (halo, vertex lists, vertex order)");
    if ((rc = layout_tiles(lists, tl, P, err))) return rc;
    if ((rc = build_finish_lists(lists, P, err))) return rc;
    timer.lap("offsets + allocation + finish lists");
    rc = fill_tiles(M, lists, opt, W, P, err);
    timer.lap("pass B (planes, ranks, colouring)");
    if (rc) return rc;
    share_index_planes(P, opt.share_index != 0, tl.nthreads);
    timer.lap("shared index planes");
    return OK;
}

int read_veg(const char *path, std::vector<float> &rest, std::vector<int32_t> &tets, std::string &err)
{
    std::ifstream in(path);
    if (!in) {
        err = std::string("cannot open ") + (path ? path : "(null)");
        return ERR_IO;
    }
    rest.clear();
    tets.clear();
    std::vector<int64_t> ids;
    std::string line;
    int mode = 0, header = 0;  // 1 = vertices, 2 = elements
    int64_t min_id = std::numeric_limits<int64_t>::max();
    while (std::getline(in, line)) {
        size_t p = line.find_first_not_of(" \t\r\n");
        if (p == std::string::npos || line[p] == '#') continue;
        if (line[p] == '*') {
            std::string key = line.substr(p);
            for (auto &ch : key) ch = char(std::toupper(static_cast<unsigned char>(ch)));
            if (key.rfind("*VERTICES", 0) == 0) {
                mode = 1;
                header = 1;
            } else if (key.rfind("*ELEMENTS", 0) == 0) {
                mode = 2;
                header = 2;
            } else {
                mode = 0;
            }
            continue;
        }
        if (!mode) continue;
        if (header) {
            --header;
            if (mode == 2 && header == 1) {
                std::string ty = line.substr(p);
                while (!ty.empty() && std::isspace(static_cast<unsigned char>(ty.back()))) ty.pop_back();
                if (ty != "TET" && ty != "TETS") {
                    err = "only TET elements are supported, got '" + ty + "'";
                    return ERR_IO;
                }
            }
            continue;
        }
        for (auto &ch : line)
            if (ch == ',') ch = ' ';
        std::istringstream ss(line);
        if (mode == 1) {
            int64_t id;
            double x, y, z;
            if (!(ss >> id >> x >> y >> z)) {
                err = "malformed vertex line: " + line;
                return ERR_IO;
            }
            min_id = std::min(min_id, id);
            rest.push_back(float(x));
            rest.push_back(float(y));
            rest.push_back(float(z));
        } else {
            int64_t id, a, b, c, d;
            if (!(ss >> id >> a >> b >> c >> d)) {
                err = "malformed element line: " + line;
                return ERR_IO;
            }
            ids.insert(ids.end(), {a, b, c, d});
        }
    }
    if (rest.empty() || ids.empty()) {
        err = "no vertices or no tet elements found";
        return ERR_IO;
    }
    const int64_t base = min_id == std::numeric_limits<int64_t>::max() ? 1 : min_id;
    tets.resize(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) tets[i] = int32_t(ids[i] - base);
    return OK;
}

}  // namespace tsamd
