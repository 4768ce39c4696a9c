// Planner internals shared by plan.cpp and partition.cpp (host only, not part of the ABI): per-worker scratch, the tile
// limits, the measure of a candidate tile, and the partitioner that cuts a tet-sphere too large for one tile.
#pragma once

#include "plan.h"

#include <cstdint>
#include <limits>
#include <vector>

namespace tsamd {

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

// owned + one-ring halo size and the number of tile vertices they touch (a vertex met by more than kMaxRank slots of
// the tile is split into several tile vertices of at most kMaxRank slots each, see build_plan)
void measure(const Mesh &M, const int32_t *owned, int64_t cnt, Scratch &S, int64_t &n_slots, int64_t &n_verts,
             std::vector<int32_t> *halo_out = nullptr);

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
