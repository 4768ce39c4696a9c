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

// what the partitioner minimises: kPartSlotWeight * slots + tile vertices (a slot streams 52 B and runs three passes; a tile
// vertex shared with another tile costs a 12-byte staging row written and read back)
constexpr int64_t kPartSlotWeight = 3;

// Cuts the face-connected tets ids[0, cnt) (centroids cen, 3 per global tet) into k face-connected parts that all fit `lim`,
// for the first k in [k_first, k_last] where that succeeds: slot-balanced k-means cells, then boundary moves between
// face-adjacent parts that lower the cost (partition.cpp).  On success `parts` holds the k parts (global
// tet ids, unordered), `cost` their summed cost, and the function returns true; false leaves `parts` empty.
bool partition_component(const Mesh &M, const Limits &lim, const float *cen, const int32_t *ids, int64_t cnt,
                         int64_t k_first, int64_t k_last, Scratch &S, std::vector<std::vector<int32_t>> &parts,
                         int64_t &cost);

}  // namespace tsamd
