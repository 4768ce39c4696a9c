// Planner internals (host only, not part of the ABI): what the stages of build_plan hand to each other.  build_plan (plan.cpp)
// is a driver that calls them in this order:
//   plan_mesh.cpp    face adjacency, the explicit operator as face weights, connected components, centroids
//   plan_tiling.cpp  components -> tiles as owned-tet lists: fit check and grouping, strict bisection, template classes,
//                    compact cells (partition.cpp), Morton order, copies inherit their template's tiles
//   plan_layout.cpp  pass A (halo, vertex lists), descriptors and offsets, finish lists
//   plan_planes.cpp  pass B, tile by tile: the index part (connectivity and item order only), then the geometry part; and
//                    the index representatives
// A stage takes its inputs as const arguments and returns a named struct; none keeps state between calls except the
// per-worker scratch (Workers).
#pragma once

#include "plan.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <limits>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace tsamd {

enum { OK = 0, ERR_INVALID = 1, ERR_BAD_MESH = 2, ERR_IO = 5, ERR_TILING = 6 };   // tsamd_status values the planner returns

// ---- tiny work-sharing helper: fn(begin, end, worker) over [0, n) in dynamic chunks ----
template <class Fn>
void parallel_chunks(int64_t n, int64_t chunk, int nthreads, Fn fn)
{
    if (n <= 0) return;
    nthreads = std::max(1, nthreads);
    if (nthreads == 1 || n <= chunk) {
        fn(int64_t(0), n, 0);
        return;
    }
    std::atomic<int64_t> next{0};
    auto body = [&](int worker) {
        for (;;) {
            int64_t b = next.fetch_add(chunk, std::memory_order_relaxed);
            if (b >= n) break;
            fn(b, std::min(n, b + chunk), worker);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(body, t);
    body(0);
    for (auto &th : pool) th.join();
}

// FNV-1a over 64-bit words
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void mix(uint64_t v) { h = (h ^ v) * 1099511628211ull; }
};

// Classes of equal items: a hash names a candidate -- the first (lowest) id that holds the same hash --, the comparison in full
// decides.  by_hash = (hash, id) of the items that take part, in any order; rep[id] = the candidate where same(id, candidate)
// holds, else id itself.  Independent of the thread count: every item is compared with the first holder only.
template <class Rep, class Same>
void classes_by_first_holder(std::vector<std::pair<uint64_t, int64_t>> &by_hash, int64_t chunk, int nthreads, Rep *rep, Same same)
{
    std::sort(by_hash.begin(), by_hash.end());
    parallel_chunks(int64_t(by_hash.size()), chunk, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; ++i) {
            const auto first = std::lower_bound(by_hash.begin(), by_hash.end(), std::make_pair(by_hash[size_t(i)].first, int64_t(0)));
            const int64_t id = by_hash[size_t(i)].second, r = first->second;
            rep[id] = Rep(r != id && same(id, r) ? r : id);
        }
    });
}

// Cf = cofactor matrix of the row-major 3x3 matrix D, returns det D: D^-1 = Cf^T / det
inline double cofactor3(const double D[9], double Cf[9])
{
    Cf[0] = D[4] * D[8] - D[5] * D[7];
    Cf[1] = D[5] * D[6] - D[3] * D[8];
    Cf[2] = D[3] * D[7] - D[4] * D[6];
    Cf[3] = D[2] * D[7] - D[1] * D[8];
    Cf[4] = D[0] * D[8] - D[2] * D[6];
    Cf[5] = D[1] * D[6] - D[0] * D[7];
    Cf[6] = D[1] * D[5] - D[2] * D[4];
    Cf[7] = D[2] * D[3] - D[0] * D[5];
    Cf[8] = D[0] * D[4] - D[1] * D[3];
    return D[0] * Cf[0] + D[1] * Cf[1] + D[2] * Cf[2];
}

// out[r] = where row r of a tile's force array begins, r < count: row r is the prefix of the tile's vertices (sorted by falling
// slot count tdeg) that more than r slots meet.  Serves the rank matching and is the row table the kernels read.
inline void row_starts(const int32_t *tdeg, int32_t n_verts, uint16_t *out, int count)
{
    int32_t start = 0, width = n_verts;
    for (int r = 0; r < count; ++r) {
        out[r] = uint16_t(start);
        while (width > 0 && tdeg[width - 1] <= r) --width;
        start += width;
    }
}

// per-worker scratch with O(1) reset through stamps
struct Scratch {
    std::vector<int32_t> tet_stamp, tet_slot, vert_stamp, vert_local;
    int32_t stamp = 0;
    void init(int64_t m, int64_t n)
    {
        if (int64_t(tet_stamp.size()) != m) {
            tet_stamp.assign(size_t(m), 0);
            tet_slot.assign(size_t(m), 0);
        }
        if (int64_t(vert_stamp.size()) != n) {
            vert_stamp.assign(size_t(n), 0);
            vert_local.assign(size_t(n), 0);
        }
    }
    int32_t next()
    {
        if (stamp > std::numeric_limits<int32_t>::max() - 8) {
            std::fill(tet_stamp.begin(), tet_stamp.end(), 0);
            std::fill(vert_stamp.begin(), vert_stamp.end(), 0);
            stamp = 0;
        }
        stamp += 2;
        return stamp;  // `stamp` marks owned, `stamp+1` marks halo
    }
};

// the host threads of one build_plan call and their scratch (sized on a worker's first use)
struct Workers {
    int nthreads;
    int64_t m, n;
    std::vector<Scratch> scratch;
    Workers(int nthreads_, int64_t m_, int64_t n_) : nthreads(nthreads_), m(m_), n(n_), scratch(size_t(nthreads_)) {}
    Scratch &operator[](int w)
    {
        scratch[size_t(w)].init(m, n);
        return scratch[size_t(w)];
    }
};

struct Limits {
    int64_t budget;
    int64_t max_spad;
    int64_t pad_unit = 4;
    bool rebuild = false;
    bool fits(int64_t n_slots, int64_t n_verts) const
    {
        const int64_t sp = (n_slots + pad_unit - 1) / pad_unit * pad_unit;
        return sp <= max_spad && n_verts <= kMaxTileVerts && tile_lds_bytes(sp, n_verts, rebuild) <= budget;
    }
};

struct Mesh {
    const float *rest;
    const int32_t *tets;
    const int32_t *nbr;
    int64_t n, m;
};

// ---- options -> limits (plan.cpp) ----
struct TilerLimits {
    int nthreads = 1, spt = kSlotsPerLane, max_threads = kTileThreads;
    Limits lim;
    int64_t s_cap = 0;       // slots a tile holds when its LDS goes to slots and their share of vertices
    int64_t target = 1;      // owned tets per tile of the non-strict bisection
    bool auto_target = true; // no explicit target_owned: look for the fewest parts that fit first
};

// ---- mesh (plan_mesh.cpp; build_adjacency is declared in plan.h) ----
// CSR -> (diagonal, one weight per tet face), double -> fp32; symmetric = the fp32 weights of every face agree both ways
int operator_face_weights(const ElementOperatorCSR &op, const int32_t *nbr, int64_t m, bool rebuild_requested,
                          std::vector<float> &diag, std::vector<float> &w, bool &symmetric, std::string &err);

// components over face adjacency, numbered by their smallest tet id; tets[start[c] .. start[c + 1]) in increasing order
struct Components {
    std::vector<int64_t> start;
    RawVector<int32_t> tets;
    int64_t count() const { return int64_t(start.size()) - 1; }
};
Components connected_components(const int32_t *nbr, int64_t m, int nthreads);

std::vector<float> tet_centroids(const Mesh &M, int nthreads);   // 3 per tet, rest state

// ---- tiling (plan_tiling.cpp) ----
// owned + one-ring halo size and the number of tile vertices they touch (a vertex met by more than kMaxRank slots of
// the tile is split into several tile vertices of at most kMaxRank slots each, see list_tile_vertices)
void measure(const Mesh &M, const int32_t *owned, int64_t cnt, Scratch &S, int64_t &n_slots, int64_t &n_verts,
             std::vector<int32_t> *halo_out = nullptr);

struct Group {   // components [cb, ce) packed into one tile, or one component that does not fit and is bisected
    int64_t cb, ce;
    bool bisect;
};
struct Tiling {
    std::vector<Group> groups;
    std::vector<std::vector<std::vector<int32_t>>> leaves;   // per group: its tiles as owned-tet lists
    std::vector<uint8_t> fitted;                             // per group: the bisection found the fewest parts that fit (strict)
    int64_t n_cut = 0, n_refined = 0, n_templates = 0;       // the three partition statistics (Plan::n_cut_components ...)
};
// The three steps of the tiling, in this order.  The bisection and the template classes reorder a component's tet list in
// place (`comps` is theirs to shuffle; the sets stay).
void group_components(const Mesh &M, const Components &comps, const Limits &lim, Workers &W, Tiling &T);
int bisect_groups(const Mesh &M, Components &comps, const std::vector<float> &cen, const TilerLimits &tl, Workers &W, Tiling &T,
                  std::string &err);
void refine_with_cells(const Mesh &M, Components &comps, const std::vector<float> &cen, const TilerLimits &tl, Workers &W, Tiling &T);

// ---- layout (plan_layout.cpp) ----
struct TileLists {   // per tile: owned tets, halo tets, tile vertices (global ids, by falling slot count) and those counts
    std::vector<std::vector<int32_t>> owned, halo, verts, vdeg;
    std::vector<int32_t> vcount;   // per global vertex: its tile-vertex copies in the whole plan
};
TileLists list_tile_vertices(const Mesh &M, std::vector<std::vector<int32_t>> owned, Workers &W);                       // pass A
int layout_tiles(const TileLists &L, const TilerLimits &tl, Plan &P, std::string &err);      // descriptors, offsets, allocation
int build_finish_lists(const TileLists &L, Plan &P, std::string &err);                       // fin_vid / fin_off / fin_idx, vdst

// ---- tile fill (plan_planes.cpp) ----
int fill_tiles(const Mesh &M, const TileLists &L, const PlanOptions &opt, Workers &W, Plan &P, std::string &err);   // pass B
void share_index_planes(Plan &P, bool share, int nthreads);                                                              // Plan::index_rep

// ---- partition.cpp ----
// What the partitioner minimises: kPartSlotWeight * slots + kPartRowWeight * staged rows, in the ratio of what the two were
// measured to cost on MI355X (profiles/r07_partition_ab.json):
//   a slot (owned or halo: 52 B streamed, pass 1, pass 3, the scatter)   ~ 13.7 ps  = 0.360 ms tile kernel / 26.24 M slots (512 x kuhn19)
//   a staged row (12 B stored by the tile kernel, read by the finish kernel)  ~ 3.9 ps  = 22.8 us finish kernel / 5.86 M rows
// i.e. 3.5 : 1.  A staged row is a tile-vertex copy of a vertex that has more than one copy in the whole plan; a vertex with a
// single copy is written straight to the gradient and costs nothing here.
constexpr int64_t kPartSlotWeight = 7;
constexpr int64_t kPartRowWeight = 2;

// The incumbent cut stands unless the new one saves at least 1 / kPartMinSavingDen = 2.5 % of its cost: alternated builds of one
// plan spread by about 0.7 % in step time (profiles/r07_partition_ab.json), a saving below three times that cannot be told
// from it, and a plan that does not change for nothing keeps its recorded traffic and timings valid.
constexpr int64_t kPartMinSavingDen = 40;

struct CutStats {
    int64_t parts = 0, slots = 0, rows = 0;
    int64_t cost() const { return kPartSlotWeight * slots + kPartRowWeight * rows; }
};

// Cuts the face-connected tets ids[0, cnt) (centroids cen, 3 per global tet) into face-connected parts that all fit `lim`:
// slot-balanced k-means cells, then Fiduccia-Mattheyses passes of boundary moves between face-adjacent parts
// (partition.cpp), for every k in [k_first, k_last]; the cheapest cut wins.  `incumbent` is the cut the caller already has (the
// bisection's leaves); its figures come back in `before`.  Returns true, with the parts (global tet ids, unordered) in `parts`
// and their figures in `after`, when a cut was found that saves at least 1 / kPartMinSavingDen of the incumbent's cost; false leaves `parts` empty
// and `after` = `before`.
bool partition_component(const Mesh &M, const Limits &lim, const float *cen, const int32_t *ids, int64_t cnt,
                         const std::vector<std::vector<int32_t>> &incumbent, int64_t k_first, int64_t k_last, int64_t slot_cap,
                         Scratch &S, std::vector<std::vector<int32_t>> &parts, CutStats &before, CutStats &after);

}  // namespace tsamd
