// Planner stage "layout": per-tile halo and vertex lists (pass A), the tile descriptors with every offset into the plan's
// arrays, and the finish lists of the vertices that more than one tile vertex stands for.  Pure C++17, no HIP.
#include "planner.h"

#include <cstring>

namespace tsamd {

// ---- pass A: per-tile halo + vertex lists, global per-vertex copy count ----
// A tile vertex is (global vertex, copy): a vertex met by more than kMaxRank slots of the tile (a hub: the cone fixture's
// centre meets ~1 500 slots of every tile) is split into copies of at most kMaxRank slots each, so that a slot's rank at a
// corner fits the six spare bits of its vertex field; the copies are staged from the same position, their partial sums
// go through the staging rows like any vertex shared by several tiles, and the finish kernel adds them up.
// Tile vertices are numbered by FALLING slot count: row r of the tile's force array (plan.h) is then the prefix of the
// vertices met by more than r slots, and the lanes of one wave of the per-vertex sum carry about the same number of rows.
namespace {

// one tile of pass A; one object per worker (its vectors are reused from tile to tile)
struct VertexLister {
    std::vector<int32_t> uniq, cnt;
    std::vector<std::pair<int32_t, int32_t>> key;   // (-slots, global vertex), in first-touch order before the sort

    void run(const Mesh &M, Scratch &S, const std::vector<int32_t> &own, std::vector<int32_t> &halo, std::vector<int32_t> &tv,
             std::vector<int32_t> &td, int32_t *vcount)
    {
        int64_t ns, nv;
        measure(M, own.data(), int64_t(own.size()), S, ns, nv, &halo);
        uniq.clear();
        cnt.clear();
        const int32_t st = S.next();
        auto touch = [&](int32_t el) {
            for (int a = 0; a < 4; ++a) {
                const int32_t v = M.tets[4 * int64_t(el) + a];
                if (S.vert_stamp[v] != st) {
                    S.vert_stamp[v] = st;
                    S.vert_local[v] = int32_t(uniq.size());
                    uniq.push_back(v);
                    cnt.push_back(0);
                }
                ++cnt[size_t(S.vert_local[v])];
            }
        };
        for (int32_t el : own) touch(el);
        for (int32_t el : halo) touch(el);
        key.clear();
        for (size_t i = 0; i < uniq.size(); ++i) {
            int32_t left = cnt[i], copies = 0;
            while (left > 0) {
                const int32_t c = std::min<int32_t>(left, kMaxRank);
                key.push_back({-c, uniq[i]});
                left -= c;
                ++copies;
            }
            __atomic_fetch_add(&vcount[uniq[i]], copies, __ATOMIC_RELAXED);   // (the other workers add to it too)
        }
        // (ties by global vertex id: the lanes that gather a tile's positions and store its gradient rows then walk runs of
        // consecutive rows of x / grad -- fewer memory transactions per wave instruction than in first-touch order)
        std::sort(key.begin(), key.end());
        tv.resize(key.size());
        td.resize(key.size());
        for (size_t i = 0; i < key.size(); ++i) {
            tv[i] = key[i].second;
            td[i] = -key[i].first;
        }
    }
};

}  // namespace

TileLists list_tile_vertices(const Mesh &M, std::vector<std::vector<int32_t>> owned, Workers &W)
{
    const size_t T = owned.size();
    TileLists L{std::move(owned), std::vector<std::vector<int32_t>>(T), std::vector<std::vector<int32_t>>(T),
                std::vector<std::vector<int32_t>>(T), std::vector<int32_t>(size_t(M.n), 0)};
    parallel_chunks(int64_t(T), 4, W.nthreads, [&](int64_t b, int64_t e, int w) {
        VertexLister lister;
        for (int64_t t = b; t < e; ++t)
            lister.run(M, W[w], L.owned[size_t(t)], L.halo[size_t(t)], L.verts[size_t(t)], L.vdeg[size_t(t)], L.vcount.data());
    });
    return L;
}

// ---- descriptors and offsets; allocates the plan's per-tile arrays (P.spt, P.n_planes are set) ----
int layout_tiles(const TileLists &L, const TilerLimits &tl, Plan &P, std::string &err)
{
    const int64_t T = int64_t(L.owned.size());
    const bool rebuild = tl.lim.rebuild;
    P.tiles.resize(size_t(T));
    P.slot_base.resize(size_t(T) + 1);
    int64_t blob_bytes = 0, vert_off = 0, stage_off = 0, slot_off = 0;
    int32_t max_quads = 1;
    // Every tile's vertex ids sit at tile * vert_stride: the kernel can issue the id load of the position gather -- the
    // head of its longest dependent chain (ids -> positions -> LDS) -- from the workgroup index alone, in parallel with
    // the tile descriptor's fetch instead of behind it (unused entries name vertex 0).
    int64_t vert_stride = 64;
    for (int64_t t = 0; t < T; ++t) vert_stride = std::max<int64_t>(vert_stride, (int64_t(L.verts[size_t(t)].size()) + 63) & ~int64_t(63));
    P.vert_stride = int32_t(vert_stride);
    for (int64_t t = 0; t < T; ++t) {
        TileDesc &d = P.tiles[size_t(t)];
        std::memset(&d, 0, sizeof(d));
        auto &tv = L.verts[size_t(t)];
        int32_t n_excl = 0;
        for (int32_t v : tv) n_excl += L.vcount[size_t(v)] == 1;
        d.n_owned = int32_t(L.owned[size_t(t)].size());
        d.n_slots = d.n_owned + int32_t(L.halo[size_t(t)].size());
        d.s_pad = int32_t((d.n_slots + tl.lim.pad_unit - 1) / tl.lim.pad_unit * tl.lim.pad_unit);
        d.n_verts = int32_t(tv.size());
        d.n_excl = n_excl;
        d.blob_off = uint64_t(blob_bytes);
        d.vert_off = int32_t(vert_off);
        d.stage_off = stage_off;
        d.n_rows = tv.empty() ? 0 : L.vdeg[size_t(t)][0];
        d.rec_base = int32_t(tile_rec_base(d.n_verts, rebuild));
        if (d.n_verts > kMaxTileVerts || 4 * int64_t(d.s_pad) > 65535) {
            err = "tile exceeds the 10-bit vertex / 16-bit entry fields of the plan";
            return ERR_TILING;
        }
        blob_bytes += (tile_rest_offset(P.n_planes, d.s_pad) + (rebuild ? 16 * int64_t(d.n_verts) : 0) + 127) & ~int64_t(127);
        vert_off += vert_stride;
        P.total_tile_verts += d.n_verts;
        stage_off += d.n_verts - d.n_excl;
        P.slot_base[size_t(t)] = slot_off;
        slot_off += d.s_pad;
        P.total_slots += d.n_slots;
        P.max_slots = std::max(P.max_slots, d.n_slots);
        P.max_verts = std::max(P.max_verts, d.n_verts);
        P.lds_bytes = std::max<int32_t>(P.lds_bytes, int32_t(tile_lds_bytes(d.s_pad, d.n_verts, rebuild)));
        max_quads = std::max(max_quads, d.s_pad / tl.spt);
        if (vert_off >= (int64_t(1) << 31)) {
            err = "too many tile vertices for 32-bit offsets";
            return ERR_TILING;
        }
    }
    P.slot_base[size_t(T)] = slot_off;
    P.n_stage = stage_off;
    P.block_threads = std::min(tl.max_threads, ((max_quads + 63) / 64) * 64);
    P.blob.resize(size_t(blob_bytes / 4));   // (uninitialised: every tile zero-fills its own range in pass B)
    P.gvid.resize(size_t(vert_off));
    P.vdst.resize(size_t(vert_off));
    P.slot_tet.resize(size_t(slot_off));
    return OK;
}

// ---- finish lists: every vertex with more than one tile-vertex copy; staging rows vertex-major, copies in tile order ----
// (tile-major rows + a gather in the finish kernel was measured: tile kernel unchanged, finish kernel 0.046 -> 0.084 ms)
int build_finish_lists(const TileLists &L, Plan &P, std::string &err)
{
    const int64_t n = int64_t(L.vcount.size()), T = int64_t(P.tiles.size());
    std::vector<int32_t> fin_of(static_cast<size_t>(n), -1);
    int64_t entries = 0;
    for (int64_t v = 0; v < n; ++v) {
        const int32_t c = L.vcount[size_t(v)];
        if (c == 1) continue;
        fin_of[size_t(v)] = int32_t(P.fin_vid.size());
        P.fin_vid.push_back(int32_t(v));
        P.fin_off.push_back(int32_t(entries));
        entries += c;
        if (entries >= (int64_t(1) << 31)) {
            err = "too many shared vertex copies for 32-bit offsets";
            return ERR_TILING;
        }
    }
    P.fin_off.push_back(int32_t(entries));
    P.fin_idx.assign(size_t(entries), 0);
    std::vector<int32_t> cur(P.fin_off.begin(), P.fin_off.end() - 1);
    for (int64_t t = 0; t < T; ++t) {
        const TileDesc &d = P.tiles[size_t(t)];
        const auto &tv = L.verts[size_t(t)];
        int64_t j = 0;
        int32_t *vd = P.vdst.data() + d.vert_off;
        for (int32_t i = 0; i < d.n_verts; ++i) {
            const int32_t v = tv[size_t(i)];
            const int32_t k = fin_of[size_t(v)];
            if (k < 0) {
                vd[i] = v;
            } else {
                const int32_t row = cur[size_t(k)]++;
                vd[i] = ~row;
                P.fin_idx[size_t(d.stage_off + j++)] = row;
            }
        }
        std::fill_n(vd + d.n_verts, size_t(P.vert_stride - d.n_verts), int32_t(0));
    }
    return OK;
}

}  // namespace tsamd
