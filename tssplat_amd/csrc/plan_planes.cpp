// Planner stage "tile fill" (pass B) and the index representatives.  A tile is filled in two parts:
//   the INDEX part is a function of the connectivity and of the item order alone -- which lane holds which item, the neighbour
//     tokens, the padding slots, corner vertices and their ranks, the row table, the order of a slot's four neighbour reads.  It
//     writes planes 0-3, the row table and slot_tet, and hands the per-slot face permutation on;
//   the GEOMETRY part writes what depends on the rest positions and the operator: gvid, Dm^-1, the operator weights in the
//     permuted order, the rest positions of a rebuild_dminv plan.
// The same tile of every copy of one template therefore carries the same index bytes (Plan::index_rep).  Pure C++17, no HIP.
#include "planner.h"

#include "conflict_opt.h"

#include <cmath>
#include <cstring>

namespace tsamd {
namespace {

// augmenting paths lanes x residues of one scatter instruction of a half-wave (TileIndexer::match_instruction)
struct RankMatcher {
    int32_t *owner, *pick;   // residue -> lane, lane -> rank
    const int32_t *lane_c;
    const std::vector<int32_t> &corner_vert;
    const std::vector<uint64_t> &unused;
    const uint16_t *row_start;
    bool seen[32];
    bool aug(int32_t l)   // augmenting path from lane l (DFS over at most 32 residues)
    {
        const int32_t v = corner_vert[size_t(lane_c[l])];
        for (uint64_t m = unused[size_t(v)]; m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const int32_t res = (int32_t(row_start[r]) + v) & 31;
            if (seen[res]) continue;
            seen[res] = true;
            if (owner[res] < 0 || aug(owner[res])) {
                owner[res] = l;
                pick[l] = r;
                return true;
            }
        }
        return false;
    }
};

// The index part of one tile; one object per worker (its vectors are reused from tile to tile).
struct TileIndexer {
    const Mesh &M;
    Scratch &S;
    const bool conflict_aware;
    const int lane_search_sweeps, spt;
    TileIndexer(const Mesh &M_, Scratch &S_, const PlanOptions &opt, int spt_)
        : M(M_), S(S_), conflict_aware(opt.conflict_aware != 0), lane_search_sweeps(opt.lane_search_sweeps), spt(spt_)
    {
    }
    // the tile at hand
    const TileDesc *d = nullptr;
    int32_t nq = 0, st = 0;
    uint32_t RB = 0;
    std::vector<int32_t> items;                   // item L (owned tets first, Morton order each) -> global tet
    std::vector<int32_t> next_rank, copy_of;      // per tile vertex: ranks handed out so far; next copy of the same vertex (-1: none)
    std::vector<int32_t> lane_nb, lane_item_at, reseated;
    std::vector<int32_t> corner_vert;             // (slot, corner) -> tile vertex, -1 on padding slots
    std::vector<uint64_t> unused;                 // per tile vertex: the ranks not handed out yet
    std::vector<uint8_t> corner_rank;

    // item L -> slot: lane L % nq takes it as its (L / nq)-th slot, so that the owned and the halo items are spread evenly over
    // the lanes and `owned` is all but wave-uniform per position
    int32_t slot_of_item(int32_t L) const { return spt * (L % nq) + L / nq; }
    // neighbour k of item L as an item (= LDS record) of this tile; a face without a usable neighbour points at the item itself
    // (halo tets only look at owned neighbours; an owned tet's neighbours are owned or halo by construction)
    int32_t neighbour_item(int32_t L, int k) const
    {
        const int32_t q = M.nbr[4 * size_t(items[size_t(L)]) + k];
        if (q >= 0 && (L < d->n_owned || S.tet_stamp[q] == st)) return lds_index(S.tet_slot[q], nq, spt);
        return L;
    }

    // the one entry point: planes 0-3 and the rest of the tile's blob range zeroed (pl, blob_bytes), the row table, slot_tet
    // (stet, s_pad entries) and face_perm[4 * slot + step] = the face of the slot's tet whose neighbour that step reads
    void run(const TileDesc &desc, const TileLists &L, int64_t t, uint32_t *pl, size_t blob_bytes, uint16_t *rowtab, int32_t *stet,
             uint8_t *face_perm);

    void number_vertices(const std::vector<int32_t> &tv);
    void seat_items();
    void search_lanes();
    void write_tokens(uint32_t *pl, int32_t *stet) const;
    void assign_corner_verts(const std::vector<int32_t> &tdeg, const int32_t *stet);
    void ranks_in_slot_order();
    void match_ranks(const uint16_t *row_start);
    void match_instruction(const int32_t *lane_c, int32_t nl, const uint16_t *row_start);
    void colour_neighbours(uint32_t *pl, uint8_t *face_perm) const;
    void colour_half_wave(int32_t pp, int32_t base, int hw, uint32_t *p2, uint32_t *p3, uint8_t *face_perm) const;
};

void TileIndexer::run(const TileDesc &desc, const TileLists &L, int64_t t, uint32_t *pl, size_t blob_bytes, uint16_t *rowtab,
                      int32_t *stet, uint8_t *face_perm)
{
    d = &desc;
    st = S.next();
    nq = d->s_pad / spt;
    RB = uint32_t(d->rec_base);
    number_vertices(L.verts[size_t(t)]);
    items.assign(L.owned[size_t(t)].begin(), L.owned[size_t(t)].end());
    items.insert(items.end(), L.halo[size_t(t)].begin(), L.halo[size_t(t)].end());
    seat_items();
    if (conflict_aware && lane_search_sweeps > 0) search_lanes();
    std::memset(pl, 0, blob_bytes);   // this tile's part of the (uninitialised) plan arrays
    std::fill_n(stet, size_t(d->s_pad), int32_t(-1));
    write_tokens(pl, stet);
    // row table: row r = the vertices met by more than r slots, a prefix of the (sorted) tile vertices
    row_starts(L.vdeg[size_t(t)].data(), d->n_verts, rowtab, kRowTabEntries);
    assign_corner_verts(L.vdeg[size_t(t)], stet);
    if (conflict_aware)
        match_ranks(rowtab);
    else
        ranks_in_slot_order();
    for (int32_t s = 0; s < d->s_pad; ++s) {   // vertex fields: local vertex + the slot's rank at it
        if (stet[s] < 0) continue;
        uint32_t lv[4];
        for (int a = 0; a < 4; ++a)
            lv[a] = uint32_t(corner_vert[4 * size_t(s) + a]) | (uint32_t(corner_rank[4 * size_t(s) + a]) << kRankShift);
        pl[0 * size_t(d->s_pad) + s] = lv[0] | (lv[1] << 16);
        pl[1 * size_t(d->s_pad) + s] = lv[2] | (lv[3] << 16);
    }
    for (size_t i = 0; i < 4 * size_t(d->s_pad); ++i) face_perm[i] = uint8_t(i & 3);
    if (conflict_aware) colour_neighbours(pl, face_perm);
}

// global vertex -> its first copy (the copies of a hub follow each other through copy_of, fullest first)
void TileIndexer::number_vertices(const std::vector<int32_t> &tv)
{
    copy_of.assign(size_t(d->n_verts), -1);
    next_rank.assign(size_t(d->n_verts), 0);
    for (int32_t i = d->n_verts - 1; i >= 0; --i) {
        const int32_t v = tv[size_t(i)];
        if (S.vert_stamp[v] == st) copy_of[size_t(i)] = S.vert_local[v];
        S.vert_stamp[v] = st;
        S.vert_local[v] = i;
    }
}

void TileIndexer::seat_items()
{
    for (int32_t L = 0; L < d->n_slots; ++L) {
        const int32_t el = items[size_t(L)];
        S.tet_stamp[el] = st + (L < d->n_owned ? 0 : 1);
        S.tet_slot[el] = slot_of_item(L);
    }
}

// which item sits on which lane of its ds_read_b128 group: local search against bank conflicts (conflict_opt.cpp)
void TileIndexer::search_lanes()
{
    lane_nb.resize(4 * size_t(d->n_slots));
    for (int32_t L = 0; L < d->n_slots; ++L)
        for (int k = 0; k < 4; ++k) lane_nb[4 * size_t(L) + k] = neighbour_item(L, k);
    search_lane_assignment(d->n_slots, d->n_owned, nq, lane_nb.data(), lane_search_sweeps, lane_item_at);
    reseated.resize(size_t(d->n_slots));
    for (int32_t L = 0; L < d->n_slots; ++L) reseated[size_t(L)] = items[size_t(lane_item_at[size_t(L)])];
    items.swap(reseated);
    for (int32_t L = 0; L < d->n_slots; ++L) S.tet_slot[items[size_t(L)]] = slot_of_item(L);   // (same tets, same stamps)
}

void TileIndexer::write_tokens(uint32_t *pl, int32_t *stet) const
{
    // padding slots: lv = 0, neighbours = the slot itself, dminv = 0 (F = 0; they write no forces: the kernels stop at n_slots)
    for (int32_t s = 0; s < d->s_pad; ++s) {
        const uint32_t f = record_token(uint32_t(lds_index(s, nq, spt)), RB);
        pl[2 * size_t(d->s_pad) + s] = f | (f << 16);
        pl[3 * size_t(d->s_pad) + s] = f | (f << 16);
    }
    for (int32_t L = 0; L < d->n_slots; ++L) {
        const int32_t s = slot_of_item(L);
        stet[s] = items[size_t(L)];
        uint32_t nb[4];
        for (int k = 0; k < 4; ++k) nb[k] = uint32_t(neighbour_item(L, k));
        pl[2 * size_t(d->s_pad) + s] = record_token(nb[0], RB) | (record_token(nb[1], RB) << 16);
        pl[3 * size_t(d->s_pad) + s] = record_token(nb[2], RB) | (record_token(nb[3], RB) << 16);
    }
}

// (slot, corner) -> tile vertex (a hub's copies are filled in slot order), ranks to be chosen
void TileIndexer::assign_corner_verts(const std::vector<int32_t> &tdeg, const int32_t *stet)
{
    corner_vert.assign(4 * size_t(d->s_pad), -1);
    corner_rank.assign(4 * size_t(d->s_pad), 0);
    unused.resize(size_t(d->n_verts));
    for (int32_t i = 0; i < d->n_verts; ++i) unused[size_t(i)] = tdeg[size_t(i)] >= 64 ? ~uint64_t(0) : ((uint64_t(1) << tdeg[size_t(i)]) - 1);
    for (int32_t s = 0; s < d->s_pad; ++s) {
        if (stet[s] < 0) continue;
        for (int a = 0; a < 4; ++a) {
            int32_t i = S.vert_local[M.tets[4 * int64_t(stet[s]) + a]];
            while (next_rank[size_t(i)] >= tdeg[size_t(i)]) i = copy_of[size_t(i)];   // this copy is full: the hub's next one
            ++next_rank[size_t(i)];
            corner_vert[4 * size_t(s) + a] = i;
        }
    }
}

void TileIndexer::ranks_in_slot_order()
{
    for (size_t c = 0; c < corner_vert.size(); ++c) {
        const int32_t i = corner_vert[c];
        if (i < 0) continue;
        corner_rank[c] = uint8_t(__builtin_ctzll(unused[size_t(i)]));
        unused[size_t(i)] &= unused[size_t(i)] - 1;
    }
}

// Which of its vertex's rows a (slot, corner) writes to is free -- it only fixes the order of the per-vertex sum -- and
// decides the LDS bank of the scattered 12-byte entry: entry = row_start[rank] + vertex, bank of its first dword =
// 3 * entry mod 32.  The 32 lanes of a half-wave that scatter corner k of their p-th slots in one instruction are
// served conflict-free when their entries differ mod 32 (3 is invertible mod 32: the dwords 3e, 3e + 1 of a
// ds_write2_b32 then load every bank exactly twice).  Handed out in slot order the entries collide 2.8x as often as
// that (kuhn19 and a.veg alike) and the scatter is bound by exactly these conflicts (profiles/r05_experiments.md); so
// per half-wave instruction a maximum matching lanes x residues (augmenting paths) picks, for every lane, one of the
// still unused ranks of its vertex; a lane left over takes the unused rank whose residue is least loaded.
void TileIndexer::match_ranks(const uint16_t *row_start)
{
    for (int32_t pp = 0; pp < spt; ++pp)
        for (int a = 0; a < 4; ++a)
            for (int32_t base = 0; base < nq; base += 32) {
                int32_t nl = 0, lane_c[32];
                for (int32_t tl = base; tl < std::min(base + 32, nq); ++tl) {
                    const size_t c = 4 * size_t(spt * tl + pp) + size_t(a);
                    if (corner_vert[c] >= 0) lane_c[nl++] = int32_t(c);
                }
                match_instruction(lane_c, nl, row_start);
            }
}

void TileIndexer::match_instruction(const int32_t *lane_c, int32_t nl, const uint16_t *row_start)
{
    int32_t owner[32], pick[32];          // residue -> lane, lane -> rank
    for (auto &o : owner) o = -1;
    for (int32_t l = 0; l < nl; ++l) pick[l] = -1;
    auto residue = [&](int32_t l, int r) { return (int32_t(row_start[r]) + corner_vert[size_t(lane_c[l])]) & 31; };
    RankMatcher matcher{owner, pick, lane_c, corner_vert, unused, row_start, {}};
    for (int32_t l = 0; l < nl; ++l) {
        std::memset(matcher.seen, 0, sizeof(matcher.seen));
        matcher.aug(l);
    }
    // (two lanes of the same vertex matched to different residues hold different ranks: same vertex + same
    // rank = same residue.)  Commit the matched lanes, then serve the others from what is left.
    int32_t load[32] = {};
    for (int32_t l = 0; l < nl; ++l)
        if (pick[l] >= 0) {
            unused[size_t(corner_vert[size_t(lane_c[l])])] &= ~(uint64_t(1) << pick[l]);
            ++load[residue(l, pick[l])];
        }
    for (int32_t l = 0; l < nl; ++l) {
        if (pick[l] >= 0) continue;
        const int32_t v = corner_vert[size_t(lane_c[l])];
        int best = -1;
        for (uint64_t m = unused[size_t(v)]; m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            if (best < 0 || load[residue(l, r)] < load[residue(l, best)]) best = r;
        }
        pick[l] = best;
        unused[size_t(v)] &= ~(uint64_t(1) << best);
        ++load[residue(l, best)];
    }
    for (int32_t l = 0; l < nl; ++l) corner_rank[size_t(lane_c[l])] = uint8_t(pick[l]);
}

// ---- LDS bank-conflict-aware neighbour order ----
// A wave reads neighbour k of 16 lanes' tets with one ds_read_b128 per 16-lane group; two lanes
// collide when their records share a 16-byte bank column, i.e. when the record indices agree
// mod 16 (48 B stride: column = 3 * idx mod 16).  The order of a tet's four neighbours is free:
// every lane group gets a proper 4-edge-colouring of its lanes x columns read graph (conflict_opt.cpp).
void TileIndexer::colour_neighbours(uint32_t *pl, uint8_t *face_perm) const
{
    uint32_t *p2 = pl + 2 * size_t(d->s_pad), *p3 = pl + 3 * size_t(d->s_pad);
    for (int32_t pp = 0; pp < spt; ++pp)
        for (int32_t base = 0; base < nq; base += 64)
            for (int hw = 0; hw < 2; ++hw) colour_half_wave(pp, base, hw, p2, p3, face_perm);
}

void TileIndexer::colour_half_wave(int32_t pp, int32_t base, int hw, uint32_t *p2, uint32_t *p3, uint8_t *face_perm) const
{
    static const int kGroups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    int32_t lane_slot[32];
    uint32_t cand[32][4];
    uint8_t group[32];
    int from[32][4];   // step `step` of lane li reads candidate from[li][step] (the weights follow: face_perm)
    int nl = 0;
    for (int gi = 2 * hw; gi < 2 * hw + 2; ++gi) {
        const int first = nl;
        for (int li = 0; li < 16; ++li) {
            const int32_t tl = base + kGroups[gi][li];
            if (tl >= nq) continue;
            const int32_t sl = spt * tl + pp;
            lane_slot[nl] = sl;
            group[nl] = uint8_t(gi & 1);
            cand[nl][0] = token_record(p2[sl] & 0xffffu, RB);
            cand[nl][1] = token_record(p2[sl] >> 16, RB);
            cand[nl][2] = token_record(p3[sl] & 0xffffu, RB);
            cand[nl][3] = token_record(p3[sl] >> 16, RB);
            ++nl;
        }
        colour_group_reads(nl - first, cand + first, 0xffffffffu, from + first);   // (no free reads: a missing face reads the slot itself)
    }
    repair_half_wave_steps(nl, group, cand, from);
    for (int li = 0; li < nl; ++li) {
        const int32_t sl = lane_slot[li];
        uint32_t chosen[4];
        for (int step = 0; step < 4; ++step) {
            chosen[step] = cand[li][from[li][step]];
            face_perm[4 * size_t(sl) + step] = uint8_t(from[li][step]);
        }
        p2[sl] = record_token(chosen[0], RB) | (record_token(chosen[1], RB) << 16);
        p3[sl] = record_token(chosen[2], RB) | (record_token(chosen[3], RB) << 16);
    }
}

// The geometry part of one tile: gvid, per slot the operator weights (planes 13..21: L[e,e], L[e,n_k], L[n_k,e], step k reading
// face face_perm[4 * slot + k]) and Dm^-1, and a rebuild_dminv plan's rest positions.  false: a singular rest tet.
bool fill_tile_geometry(const Mesh &M, const Plan &P, const TileDesc &d, const std::vector<int32_t> &tv, const int32_t *stet,
                        const uint8_t *face_perm, uint32_t *pl, int32_t *gvid)
{
    const bool rebuild = P.n_planes == kPlanesRebuild, weighted = P.n_planes > kPlanes;
    const int32_t nq = d.s_pad / P.spt;
    const uint32_t RB = uint32_t(d.rec_base);
    const size_t sp = size_t(d.s_pad);
    bool regular = true;
    std::copy(tv.begin(), tv.end(), gvid);
    std::fill_n(gvid + d.n_verts, size_t(P.vert_stride - d.n_verts), int32_t(0));   // unused entries: vertex 0
    for (int32_t s = 0; s < d.s_pad; ++s) {
        const int32_t el = stet[s];
        if (el < 0) continue;
        auto putf = [&](int plane, float v) { std::memcpy(&pl[size_t(plane) * sp + s], &v, 4); };
        if (weighted) {
            const uint32_t self = uint32_t(lds_index(s, nq, P.spt));
            const uint32_t tok[4] = {pl[2 * sp + s] & 0xffffu, pl[2 * sp + s] >> 16, pl[3 * sp + s] & 0xffffu, pl[3 * sp + s] >> 16};
            putf(13, P.op_diag[size_t(el)]);
            for (int k = 0; k < 4; ++k) {
                const int f = face_perm[4 * size_t(s) + k];
                const int32_t q = M.nbr[4 * size_t(el) + f];
                float wr = 0.f, wc = 0.f;
                if (q >= 0 && token_record(tok[k], RB) != self) {   // (a face without a usable neighbour reads the slot itself)
                    wr = P.op_w[4 * size_t(el) + f];
                    for (int g = 0; g < 4; ++g)
                        if (M.nbr[4 * size_t(q) + g] == el) wc = P.op_w[4 * size_t(q) + g];
                }
                putf(14 + k, wr);
                if (P.n_planes == kPlanesWeighted) putf(18 + k, wc);   // (symmetric operator: no column-weight planes)
            }
        }
        // Dm^-1 in double from the fp32 rest positions, rounded to fp32
        const int32_t *tt = M.tets + 4 * int64_t(el);
        double D[9], Cf[9];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k)
                D[3 * i + k] = double(M.rest[3 * size_t(tt[k + 1]) + i]) - double(M.rest[3 * size_t(tt[0]) + i]);
        const double det = cofactor3(D, Cf);
        if (det == 0.0 || !std::isfinite(det)) {
            regular = false;
            continue;
        }
        if (!rebuild)
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k) putf(4 + 3 * i + k, float(Cf[3 * k + i] / det));   // inverse = cofactor^T / det
    }
    if (rebuild) {   // the tile's rest positions, tile vertex order, one float4 each
        float *rp = reinterpret_cast<float *>(reinterpret_cast<uint8_t *>(pl) + tile_rest_offset(P.n_planes, d.s_pad));
        for (int32_t v = 0; v < d.n_verts; ++v) {
            const float *r = M.rest + 3 * size_t(tv[size_t(v)]);
            rp[4 * v + 0] = r[0];
            rp[4 * v + 1] = r[1];
            rp[4 * v + 2] = r[2];
            rp[4 * v + 3] = 0.f;
        }
    }
    return regular;
}

}  // namespace

// ---- pass B: fill planes ----
int fill_tiles(const Mesh &M, const TileLists &L, const PlanOptions &opt, Workers &W, Plan &P, std::string &err)
{
    const int64_t T = int64_t(P.tiles.size());
    std::atomic<int> singular{0};
    parallel_chunks(T, 2, W.nthreads, [&](int64_t b, int64_t e, int w) {
        TileIndexer index(M, W[w], opt, P.spt);
        std::vector<uint8_t> face_perm;
        for (int64_t t = b; t < e; ++t) {
            const TileDesc &d = P.tiles[size_t(t)];
            uint32_t *pl = P.blob.data() + d.blob_off / 4;
            const uint64_t blob_end = t + 1 < T ? P.tiles[size_t(t) + 1].blob_off : uint64_t(P.blob.size()) * 4;
            uint16_t *rowtab = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(pl) + tile_rowtab_offset(P.n_planes, d.s_pad));
            int32_t *stet = P.slot_tet.data() + P.slot_base[size_t(t)];
            face_perm.resize(4 * size_t(d.s_pad));
            index.run(d, L, t, pl, size_t(blob_end - d.blob_off), rowtab, stet, face_perm.data());
            if (!fill_tile_geometry(M, P, d, L.verts[size_t(t)], stet, face_perm.data(), pl, P.gvid.data() + d.vert_off)) singular.store(1);
        }
    });
    if (!singular.load()) return OK;
    err = "singular (zero-volume) rest tetrahedron";
    return ERR_BAD_MESH;
}

// ---- shared index planes: which earlier tile carries the same index planes and row table? (Plan::index_rep) ----
// A hash of the descriptor's shape fields, planes 0-3 and the row table names a candidate -- the first tile of the plan with
// that hash --, the comparison in full decides.  Tile by tile over the finished bytes: independent of the thread count.
void share_index_planes(Plan &P, bool share, int nthreads)
{
    const int64_t T = int64_t(P.tiles.size());
    P.index_rep.resize(size_t(T));
    for (int64_t t = 0; t < T; ++t) P.index_rep[size_t(t)] = int32_t(t);
    if (!share || T <= 1) return;
    const size_t rowtab_words = 2 * kRowTabEntries / 4;
    auto rowtab_of = [&](const TileDesc &d) { return P.blob.data() + (d.blob_off + uint64_t(tile_rowtab_offset(P.n_planes, d.s_pad))) / 4; };
    std::vector<std::pair<uint64_t, int64_t>> by_hash(static_cast<size_t>(T));
    parallel_chunks(T, 16, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t t = b; t < e; ++t) {
            const TileDesc &d = P.tiles[size_t(t)];
            Fnv f;
            f.mix(uint64_t(d.s_pad));
            f.mix(uint64_t(d.n_slots));
            f.mix(uint64_t(d.n_owned));
            f.mix(uint64_t(d.n_verts));
            const uint32_t *pl = P.blob.data() + d.blob_off / 4, *rt = rowtab_of(d);
            for (size_t i = 0; i < size_t(kPlanesRebuild) * size_t(d.s_pad); ++i) f.mix(pl[i]);
            for (size_t i = 0; i < rowtab_words; ++i) f.mix(rt[i]);
            by_hash[size_t(t)] = {f.h, t};
        }
    });
    classes_by_first_holder(by_hash, 16, nthreads, P.index_rep.data(), [&](int64_t t, int64_t r) {
        const TileDesc &d = P.tiles[size_t(t)], &dr = P.tiles[size_t(r)];
        return d.s_pad == dr.s_pad && d.n_slots == dr.n_slots && d.n_owned == dr.n_owned && d.n_verts == dr.n_verts && d.n_rows == dr.n_rows &&
               d.rec_base == dr.rec_base &&
               std::memcmp(P.blob.data() + d.blob_off / 4, P.blob.data() + dr.blob_off / 4, size_t(kPlanesRebuild) * size_t(d.s_pad) * 4) == 0 &&
               std::memcmp(rowtab_of(d), rowtab_of(dr), 2 * kRowTabEntries) == 0;
    });
    for (int64_t t = 0; t < T; ++t) P.n_index_shared += P.index_rep[size_t(t)] != t;
}

}  // namespace tsamd
