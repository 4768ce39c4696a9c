// Planner stage "tiling": components -> tiles as owned-tet lists.  Small components are packed together, a component too large
// for one tile is bisected along its longest axis into the fewest parts that fit, re-cut into compact cells (partition.cpp)
// where that is cheaper, and ordered along a Morton curve; the copies of one template take their template's tiles over.
// Pure C++17, no HIP.
#include "planner.h"

#include <cmath>

namespace tsamd {

// owned + one-ring halo size and the number of tile vertices they touch (a vertex met by more than kMaxRank slots of
// the tile is split into several tile vertices of at most kMaxRank slots each, see list_tile_vertices)
void measure(const Mesh &M, const int32_t *owned, int64_t cnt, Scratch &S, int64_t &n_slots, int64_t &n_verts,
             std::vector<int32_t> *halo_out)
{
    const int32_t so = S.next(), sh = so + 1;
    for (int64_t i = 0; i < cnt; ++i) S.tet_stamp[owned[i]] = so;
    int64_t halo = 0, verts = 0;
    if (halo_out) halo_out->clear();
    auto touch = [&](int32_t e) {
        for (int a = 0; a < 4; ++a) {
            int32_t v = M.tets[4 * int64_t(e) + a];
            if (S.vert_stamp[v] != so) {
                S.vert_stamp[v] = so;
                S.vert_local[v] = 1;
                ++verts;
            } else if (S.vert_local[v]++ % kMaxRank == 0) {
                ++verts;
            }
        }
    };
    for (int64_t i = 0; i < cnt; ++i) {
        const int32_t e = owned[i];
        touch(e);
        for (int k = 0; k < 4; ++k) {
            int32_t q = M.nbr[4 * int64_t(e) + k];
            if (q < 0) continue;
            int32_t st = S.tet_stamp[q];
            if (st == so || st == sh) continue;
            S.tet_stamp[q] = sh;
            ++halo;
            if (halo_out) halo_out->push_back(q);
            touch(q);
        }
    }
    n_slots = cnt + halo;
    n_verts = verts;
}

namespace {

inline uint32_t spread10(uint32_t v)
{
    v &= 0x3ff;
    v = (v | (v << 16)) & 0x030000ff;
    v = (v | (v << 8)) & 0x0300f00f;
    v = (v | (v << 4)) & 0x030c30c3;
    v = (v | (v << 2)) & 0x09249249;
    return v;
}

struct Splitter {
    const Mesh &M;
    const Limits &lim;
    const std::vector<float> &cen;  // 3 per tet
    Scratch &S;
    std::vector<std::vector<int32_t>> &out;
    std::string &err;
    int rc = OK;
    bool strict = false;  // strict: a leaf that does not fit aborts the attempt (caller retries with more parts)
    bool failed = false;

    void bbox(const int32_t *ids, int64_t cnt, float lo[3], float hi[3]) const
    {
        for (int d = 0; d < 3; ++d) {
            lo[d] = std::numeric_limits<float>::max();
            hi[d] = -std::numeric_limits<float>::max();
        }
        for (int64_t i = 0; i < cnt; ++i)
            for (int d = 0; d < 3; ++d) {
                float c = cen[3 * size_t(ids[i]) + d];
                lo[d] = std::min(lo[d], c);
                hi[d] = std::max(hi[d], c);
            }
    }

    void emit(int32_t *ids, int64_t cnt)
    {
        // order the leaf along a Morton curve so that lanes of a wave hold nearby tets
        float lo[3], hi[3];
        bbox(ids, cnt, lo, hi);
        std::vector<std::pair<uint32_t, int32_t>> key(static_cast<size_t>(cnt));
        for (int64_t i = 0; i < cnt; ++i) {
            uint32_t code = 0;
            for (int d = 0; d < 3; ++d) {
                float ext = hi[d] - lo[d];
                float u = ext > 0 ? (cen[3 * size_t(ids[i]) + d] - lo[d]) / ext : 0.f;
                code |= spread10(uint32_t(std::min(1023.f, u * 1023.f))) << d;
            }
            key[size_t(i)] = {code, ids[i]};
        }
        std::sort(key.begin(), key.end());
        std::vector<int32_t> t(static_cast<size_t>(cnt));
        for (int64_t i = 0; i < cnt; ++i) t[size_t(i)] = key[size_t(i)].second;
        out.push_back(std::move(t));
    }

    void split(int32_t *ids, int64_t cnt, int64_t k)
    {
        if (rc || failed) return;
        if (k <= 1) {
            int64_t ns, nv;
            measure(M, ids, cnt, S, ns, nv);
            if (lim.fits(ns, nv)) {
                emit(ids, cnt);
                return;
            }
            if (strict) {
                failed = true;
                return;
            }
            if (cnt <= 1) {
                err = "a single tet with its face neighbours exceeds the LDS budget";
                rc = ERR_TILING;
                return;
            }
            k = 2;
        }
        float lo[3], hi[3];
        bbox(ids, cnt, lo, hi);
        int ax = 0;
        for (int d = 1; d < 3; ++d)
            if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
        const int64_t k1 = k / 2;
        int64_t mid = cnt * k1 / k;
        mid = std::max<int64_t>(1, std::min(cnt - 1, mid));
        std::nth_element(ids, ids + mid, ids + cnt, [&](int32_t a, int32_t b) {
            float ca = cen[3 * size_t(a) + ax], cb = cen[3 * size_t(b) + ax];
            return ca != cb ? ca < cb : a < b;
        });
        split(ids, mid, k1);
        split(ids + mid, cnt - mid, k - k1);
    }
};

}  // namespace

// ---- which components fit into one tile as they are (no halo)?  pack those together, bisect the others ----
void group_components(const Mesh &M, const Components &comps, const Limits &lim, Workers &W, Tiling &T)
{
    const int64_t C = comps.count();
    std::vector<int64_t> comp_verts(static_cast<size_t>(C), 0);
    std::vector<uint8_t> comp_fits(static_cast<size_t>(C), 0);
    parallel_chunks(C, 16, W.nthreads, [&](int64_t b, int64_t e, int w) {
        Scratch &S = W[w];
        for (int64_t c = b; c < e; ++c) {
            int64_t cnt = comps.start[c + 1] - comps.start[c], ns, nv;
            if (cnt > lim.max_spad) continue;
            measure(M, comps.tets.data() + comps.start[c], cnt, S, ns, nv);
            comp_verts[size_t(c)] = nv;
            comp_fits[size_t(c)] = lim.fits(ns, nv) ? 1 : 0;
        }
    });
    int64_t c = 0;
    while (c < C) {
        if (!comp_fits[size_t(c)]) {
            T.groups.push_back({c, c + 1, true});
            ++c;
            continue;
        }
        int64_t tets_sum = 0, verts_sum = 0, ce = c;
        while (ce < C && comp_fits[size_t(ce)]) {
            int64_t t2 = tets_sum + (comps.start[ce + 1] - comps.start[ce]);
            int64_t v2 = verts_sum + comp_verts[size_t(ce)];  // upper bound on the union
            if (ce > c && !lim.fits(t2, v2)) break;
            tets_sum = t2;
            verts_sum = v2;
            ++ce;
        }
        T.groups.push_back({c, ce, false});
        c = ce;
    }
}

namespace {

// the tets of a group, a run of the components' tet list
int32_t *group_ids(Components &comps, const Group &G, int64_t &cnt)
{
    cnt = comps.start[G.ce] - comps.start[G.cb];
    return comps.tets.data() + comps.start[G.cb];
}

// Fewest parts whose tiles all fit: start optimistic (owned ~ 0.85 of the slot capacity) and add
// parts until no leaf overflows -- splitting an overflowing leaf in two would leave half-empty tiles.
bool bisect_strictly(Splitter &sp, int32_t *ids, int64_t cnt, int64_t s_cap)
{
    bool done = false;
    int64_t k = std::max<int64_t>(2, (cnt + int64_t(0.85 * double(s_cap)) - 1) / int64_t(0.85 * double(s_cap)));
    for (int attempt = 0; attempt < 24 && !done; ++attempt) {
        sp.out.clear();
        sp.strict = true;
        sp.failed = false;
        sp.split(ids, cnt, k);
        done = !sp.failed && !sp.rc;
        k = std::max<int64_t>(k + 1, (k * 103 + 99) / 100);
    }
    if (!done) sp.out.clear();
    sp.strict = false;
    sp.failed = false;
    return done;
}

}  // namespace

int bisect_groups(const Mesh &M, Components &comps, const std::vector<float> &cen, const TilerLimits &tl, Workers &W, Tiling &T,
                  std::string &err)
{
    T.leaves.assign(T.groups.size(), {});
    T.fitted.assign(T.groups.size(), 0);
    std::atomic<int> first_rc{0};
    std::string split_err;
    std::atomic<bool> err_set{false};
    parallel_chunks(int64_t(T.groups.size()), 1, W.nthreads, [&](int64_t b, int64_t e, int w) {
        Scratch &S = W[w];
        for (int64_t g = b; g < e; ++g) {
            int64_t cnt;
            int32_t *ids = group_ids(comps, T.groups[size_t(g)], cnt);
            if (!T.groups[size_t(g)].bisect) {
                T.leaves[size_t(g)].emplace_back(ids, ids + cnt);
                continue;
            }
            std::string local_err;
            Splitter sp{M, tl.lim, cen, S, T.leaves[size_t(g)], local_err};
            const bool done = tl.auto_target && bisect_strictly(sp, ids, cnt, tl.s_cap);
            T.fitted[size_t(g)] = done ? 1 : 0;
            if (!done) sp.split(ids, cnt, (cnt + tl.target - 1) / tl.target);
            if (sp.rc) {
                first_rc.store(sp.rc);
                bool expected = false;
                if (err_set.compare_exchange_strong(expected, true)) split_err = local_err;
            }
        }
    });
    if (first_rc.load()) err = split_err;
    return first_rc.load();
}

// ---- partition: compact cells with fewer halo slots (partition.cpp) where the bisection found a strict fit ----
// k runs upward from the bisection's slots over the slot capacity, at most four values and never past the bisection's own
// count; the cheapest cut of those replaces the bisection's leaves when it costs less than they do (kPartSlotWeight * slots +
// kPartRowWeight * staged rows).  Otherwise the bisection stands: the plan is never worse than it.  No cell may need more LDS
// than the largest tile of the bisection, so the launch (dynamic LDS, workgroups per CU) stays as it was.
//
// Batches repeat one template (the reference places copies of one tet-sphere too), and a cut only depends on the
// connectivity and, through the seeds, on the shape of the rest centroids.  So components are sorted into classes -- the same
// tets over the same vertices up to an offset of the ids, rest positions equal up to a translation and a uniform scale,
// both compared in full, not assumed --, the first component of a class is cut, and the others take its cut over.
namespace {

// the LDS the largest tile of the bisection needs, capped by the budget
int64_t largest_leaf_lds(const Mesh &M, const Limits &lim, Workers &W, const Tiling &T)
{
    std::vector<int64_t> rcb_lds(T.groups.size(), 0);
    parallel_chunks(int64_t(T.groups.size()), 16, W.nthreads, [&](int64_t b, int64_t e, int w) {
        Scratch &S = W[w];
        for (int64_t g = b; g < e; ++g)
            for (const auto &l : T.leaves[size_t(g)]) {
                int64_t ns, nv;
                measure(M, l.data(), int64_t(l.size()), S, ns, nv);
                const int64_t sp = (ns + lim.pad_unit - 1) / lim.pad_unit * lim.pad_unit;
                rcb_lds[size_t(g)] = std::max(rcb_lds[size_t(g)], tile_lds_bytes(sp, nv, lim.rebuild));
            }
    });
    int64_t budget = 0;
    for (int64_t l : rcb_lds) budget = std::max(budget, std::min(lim.budget, l));
    return budget;
}

// what names a component's class: a hash of the connectivity relative to the component's first tet and lowest vertex
struct Shape {
    int32_t vbase = 0;
    uint64_t hash = 0;
    double lo[3], hi[3];
};

Shape shape_of(const Mesh &M, const int32_t *ids, int64_t cnt)
{
    Shape sh;
    sh.vbase = std::numeric_limits<int32_t>::max();
    for (int d = 0; d < 3; ++d) {
        sh.lo[d] = std::numeric_limits<double>::max();
        sh.hi[d] = -std::numeric_limits<double>::max();
    }
    for (int64_t i = 0; i < cnt; ++i)
        for (int a = 0; a < 4; ++a) {
            const int32_t v = M.tets[4 * int64_t(ids[i]) + a];
            sh.vbase = std::min(sh.vbase, v);
            for (int d = 0; d < 3; ++d) {
                sh.lo[d] = std::min(sh.lo[d], double(M.rest[3 * size_t(v) + d]));
                sh.hi[d] = std::max(sh.hi[d], double(M.rest[3 * size_t(v) + d]));
            }
        }
    Fnv f{Fnv().h ^ uint64_t(cnt)};
    for (int64_t i = 0; i < cnt; ++i) {
        f.mix(uint64_t(ids[i] - ids[0]));
        for (int a = 0; a < 4; ++a) f.mix(uint64_t(M.tets[4 * int64_t(ids[i]) + a] - sh.vbase));
    }
    sh.hash = f.h;
    return sh;
}

// the comparison in full: same tets over the same vertices up to an offset, rest positions up to a translation and a scale
bool same_shape(const Mesh &M, const int32_t *ids, int64_t cnt, const Shape &sg, const int32_t *ids_r, int64_t cnt_r, const Shape &sr)
{
    constexpr double kSimilarTol = 1e-4;   // of the component's extent; fp32 rounding of a placed copy is some 1e-6 of it
    bool same = cnt == cnt_r;
    double ext_g = 0.0, ext_r = 0.0;
    for (int d = 0; d < 3; ++d) {
        ext_g = std::max(ext_g, sg.hi[d] - sg.lo[d]);
        ext_r = std::max(ext_r, sr.hi[d] - sr.lo[d]);
    }
    same = same && ext_g > 0.0 && ext_r > 0.0;
    const double scale = same ? ext_g / ext_r : 1.0;
    for (int64_t i = 0; i < cnt && same; ++i) {
        same = ids[i] - ids[0] == ids_r[i] - ids_r[0];
        for (int a = 0; a < 4 && same; ++a) {
            const int32_t v = M.tets[4 * int64_t(ids[i]) + a], vr = M.tets[4 * int64_t(ids_r[i]) + a];
            same = v - sg.vbase == vr - sr.vbase;
            for (int d = 0; d < 3 && same; ++d)
                same = std::fabs((double(M.rest[3 * size_t(v) + d]) - sg.lo[d]) - scale * (double(M.rest[3 * size_t(vr) + d]) - sr.lo[d])) <= kSimilarTol * ext_g;
        }
    }
    return same;
}

// model[g] = the component whose cut g takes over (itself: it is cut; -1: not cut at all)
std::vector<int64_t> template_classes(const Mesh &M, Components &comps, const Tiling &T, int nthreads)
{
    const int64_t G = int64_t(T.groups.size());
    std::vector<Shape> shape(static_cast<size_t>(G));
    parallel_chunks(G, 1, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t g = b; g < e; ++g) {
            if (!T.fitted[size_t(g)]) continue;
            int64_t cnt;
            int32_t *ids = group_ids(comps, T.groups[size_t(g)], cnt);
            std::sort(ids, ids + cnt);   // (the bisection has shuffled them: back to increasing order, the same in every copy)
            shape[size_t(g)] = shape_of(M, ids, cnt);
        }
    });
    std::vector<int64_t> model(static_cast<size_t>(G), -1);
    std::vector<std::pair<uint64_t, int64_t>> by_hash;
    for (int64_t g = 0; g < G; ++g)
        if (T.fitted[size_t(g)]) by_hash.push_back({shape[size_t(g)].hash, g});
    classes_by_first_holder(by_hash, 1, nthreads, model.data(), [&](int64_t g, int64_t r) {
        int64_t cnt, cnt_r;
        const int32_t *ids = group_ids(comps, T.groups[size_t(g)], cnt), *ids_r = group_ids(comps, T.groups[size_t(r)], cnt_r);
        return same_shape(M, ids, cnt, shape[size_t(g)], ids_r, cnt_r, shape[size_t(r)]);
    });
    return model;
}

}  // namespace

void refine_with_cells(const Mesh &M, Components &comps, const std::vector<float> &cen, const TilerLimits &tl, Workers &W, Tiling &T)
{
    const int64_t G = int64_t(T.groups.size());
    Limits cell_lim = tl.lim;
    cell_lim.budget = largest_leaf_lds(M, tl.lim, W, T);
    const std::vector<int64_t> model = template_classes(M, comps, T, W.nthreads);
    std::vector<std::vector<std::vector<int32_t>>> cut(static_cast<size_t>(G));   // of the components that are cut themselves
    std::vector<uint8_t> refined(static_cast<size_t>(G), 0);
    parallel_chunks(G, 1, W.nthreads, [&](int64_t b, int64_t e, int w) {
        Scratch &S = W[w];
        for (int64_t g = b; g < e; ++g) {
            if (model[size_t(g)] != g) continue;
            int64_t cnt;
            const int32_t *ids = group_ids(comps, T.groups[size_t(g)], cnt);
            const auto &leaves = T.leaves[size_t(g)];
            const int64_t k_rcb = int64_t(leaves.size());
            int64_t rcb_slots = 0;
            for (const auto &l : leaves) {
                int64_t ns, nv;
                measure(M, l.data(), int64_t(l.size()), S, ns, nv);
                rcb_slots += ns;
            }
            const int64_t k_lo = (rcb_slots + tl.s_cap - 1) / tl.s_cap;
            CutStats before, after;
            refined[size_t(g)] = partition_component(M, cell_lim, cen.data(), ids, cnt, leaves, k_lo, std::min(k_rcb, k_lo + 3), tl.s_cap, S, cut[size_t(g)], before, after) ? 1 : 0;
        }
    });
    for (int64_t g = 0; g < G; ++g) {
        if (model[size_t(g)] < 0) continue;
        ++T.n_cut;
        T.n_templates += model[size_t(g)] == g;
        T.n_refined += refined[size_t(model[size_t(g)])];
    }
    // The components that were cut themselves order their cells along the Morton curve of their own centroids ...
    parallel_chunks(G, 1, W.nthreads, [&](int64_t b, int64_t e, int w) {
        Scratch &S = W[w];
        std::vector<int32_t> part;
        for (int64_t g = b; g < e; ++g) {
            if (model[size_t(g)] != g || !refined[size_t(g)]) continue;
            auto &leaves = T.leaves[size_t(g)];
            leaves.clear();
            std::string unused_err;
            Splitter sp{M, tl.lim, cen, S, leaves, unused_err};
            for (const auto &c : cut[size_t(g)]) {
                part.assign(c.begin(), c.end());
                sp.emit(part.data(), int64_t(part.size()));
            }
        }
    });
    // ... and their copies take the TILES over, tet for tet in the same order, not just the cut: a copy that sorted its cells by
    // its own fp32 centroids (or kept its own bisection) broke a tie of the Morton codes differently in 2-3 % of its tiles, and
    // everything behind the item order -- halo order, lanes, ranks, colouring, vertex numbering -- is a function of that order and
    // of the connectivity alone.  With the order inherited a copy's index planes and row tables are the template's, byte for
    // byte (Plan::index_rep, decided by comparison in share_index_planes).
    parallel_chunks(G, 1, W.nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t g = b; g < e; ++g) {
            const int64_t r = model[size_t(g)];
            if (r < 0 || r == g) continue;
            int64_t cnt, cnt_r;
            const int32_t *ids = group_ids(comps, T.groups[size_t(g)], cnt), *ids_r = group_ids(comps, T.groups[size_t(r)], cnt_r);
            const int32_t shift = ids[0] - ids_r[0];
            auto &leaves = T.leaves[size_t(g)];
            leaves = T.leaves[size_t(r)];
            for (auto &l : leaves)
                for (int32_t &el : l) el += shift;
        }
    });
}

}  // namespace tsamd
