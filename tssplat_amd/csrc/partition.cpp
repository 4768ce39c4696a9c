// Partition of one tet-sphere that does not fit into a single tile.
//
// What a tile costs the energy kernels is its SLOTS -- the owned tets plus the one-ring face halo, each streamed (52 B) and run
// through pass 1, pass 3 and the scatter -- and its tile vertices, whose partial sums go through the staging rows when another
// tile meets the vertex too (plan.h).  Both grow with the surface between tiles, and the recursive coordinate bisection of
// build_plan cuts slabs with a lot of surface.  Here the sphere is cut into compact cells instead:
//   1. seed k cells with the bisection of the rest centroids by tet count;
//   2. slot-balanced Lloyd iterations: every tet joins the cell of least |x - c|^2 - w among the centres nearest its own cell's,
//      and the weight w of a cell falls when it holds more slots than the mean (a power diagram);
//   3. every cell keeps its largest face-connected piece, the other pieces join the neighbouring cells;
//   4. boundary moves between face-adjacent cells (Fiduccia-Mattheyses style, greedy): first out of every cell that does not fit
//      until it fits, then any move that lowers kPartSlotWeight * slots + tile vertices and keeps both cells fitting and face-connected.
// Everything runs in one thread per sphere over local indices in a fixed order, so the result does not depend on the number of
// host threads.  A cell's slot count and tile vertices (kMaxRank slots per tile vertex, as measure() counts them) are kept
// exact under every move through per-(cell, vertex) slot counts.
#include "partition.h"

#include <algorithm>
#include <cmath>

namespace tsamd {
namespace {

constexpr int kLloydIters = 12;
constexpr int kLloydFull = 4;                // of which assign every tet (the others: tets on a cell boundary)
constexpr int kCandidates = 8;               // centres a tet looks at: the nearest ones to its own cell's centre
constexpr int kImproveSweeps = 6;
constexpr int kConnectProbe = 512;           // tets a connectivity probe may visit before it refuses the move
constexpr int64_t kMaxIncidence = int64_t(1) << 23;   // (cells x vertices) counts one sphere may allocate

inline int64_t copies(int64_t c) { return (c + kMaxRank - 1) / kMaxRank; }

struct Part {
    const Limits &lim;
    int64_t cnt = 0, nv = 0, k = 0;
    std::vector<int32_t> nb;      // 4 per tet: local face neighbour, -1 = none
    std::vector<int32_t> lv;      // 4 per tet: local vertex
    std::vector<double> x;        // 3 per tet: rest centroid
    std::vector<int32_t> part;    // cell of every tet
    std::vector<int64_t> owned, slots, verts;
    std::vector<int32_t> inc;     // k x nv: slots of the cell that meet the vertex
    std::vector<int32_t> mark, queue;
    int32_t stamp = 0;

    explicit Part(const Limits &l) : lim(l) {}

    int64_t cost(int64_t p) const { return kPartSlotWeight * slots[size_t(p)] + verts[size_t(p)]; }
    bool fits(int64_t p) const { return lim.fits(slots[size_t(p)], verts[size_t(p)]); }

    // ---- 1. bisection seed ----
    void seed(int32_t *idx, int64_t n, int64_t kk, int32_t &next)
    {
        if (kk <= 1) {
            for (int64_t i = 0; i < n; ++i) part[size_t(idx[i])] = next;
            ++next;
            return;
        }
        double lo[3], hi[3];
        for (int d = 0; d < 3; ++d) {
            lo[d] = std::numeric_limits<double>::max();
            hi[d] = -std::numeric_limits<double>::max();
        }
        for (int64_t i = 0; i < n; ++i)
            for (int d = 0; d < 3; ++d) {
                lo[d] = std::min(lo[d], x[3 * size_t(idx[i]) + d]);
                hi[d] = std::max(hi[d], x[3 * size_t(idx[i]) + d]);
            }
        int ax = 0;
        for (int d = 1; d < 3; ++d)
            if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
        const int64_t k1 = kk / 2;
        const int64_t mid = std::max<int64_t>(1, std::min(n - 1, n * k1 / kk));
        std::nth_element(idx, idx + mid, idx + n, [&](int32_t a, int32_t b) {
            const double ca = x[3 * size_t(a) + ax], cb = x[3 * size_t(b) + ax];
            return ca != cb ? ca < cb : a < b;
        });
        seed(idx, mid, k1, next);
        seed(idx + mid, n - mid, kk - k1, next);
    }

    // slots (owned + halo) of every cell, from `part` alone
    void count_slots(std::vector<int64_t> &s) const
    {
        s.assign(size_t(k), 0);
        for (int64_t q = 0; q < cnt; ++q) {
            const int32_t pq = part[size_t(q)];
            ++s[size_t(pq)];
            int32_t seen[4];
            int ns = 0;
            for (int f = 0; f < 4; ++f) {
                const int32_t r = nb[4 * size_t(q) + f];
                if (r < 0) continue;
                const int32_t pr = part[size_t(r)];
                if (pr == pq || std::find(seen, seen + ns, pr) != seen + ns) continue;
                seen[ns++] = pr;
                ++s[size_t(pr)];
            }
        }
    }

    // ---- 2. slot-balanced Lloyd iterations ----
    void lloyd()
    {
        const size_t K = static_cast<size_t>(k);
        std::vector<double> c(3 * K, 0.0), w(K, 0.0), d2c(K);
        std::vector<int64_t> n_in(K), s;
        std::vector<int32_t> cand(K * kCandidates), order(K), next(static_cast<size_t>(cnt));
        const int nc = int(std::min<int64_t>(k, kCandidates));
        for (int it = 0; it < kLloydIters; ++it) {
            std::fill(n_in.begin(), n_in.end(), 0);
            std::vector<double> sum(3 * size_t(k), 0.0);
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t p = part[size_t(e)];
                ++n_in[size_t(p)];
                for (int d = 0; d < 3; ++d) sum[3 * size_t(p) + d] += x[3 * size_t(e) + d];
            }
            for (int64_t p = 0; p < k; ++p)
                if (n_in[size_t(p)] > 0)   // (an emptied cell keeps its centre)
                    for (int d = 0; d < 3; ++d) c[3 * size_t(p) + d] = sum[3 * size_t(p) + d] / double(n_in[size_t(p)]);
            // weights: a cell with more slots than the mean shrinks, in units of the mean squared distance to the centres
            count_slots(s);
            double r2 = 0.0;
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t p = part[size_t(e)];
                for (int d = 0; d < 3; ++d) {
                    const double t = x[3 * size_t(e) + d] - c[3 * size_t(p) + d];
                    r2 += t * t;
                }
            }
            r2 /= double(std::max<int64_t>(1, cnt));
            int64_t s_sum = 0, live = 0;
            for (int64_t p = 0; p < k; ++p)
                if (n_in[size_t(p)] > 0) {
                    s_sum += s[size_t(p)];
                    ++live;
                }
            const double s_mean = double(s_sum) / double(std::max<int64_t>(1, live));
            for (int64_t p = 0; p < k; ++p) w[size_t(p)] += 0.5 * r2 * (s_mean - double(s[size_t(p)])) / s_mean;
            // candidate centres of every cell: its nc nearest (itself first)
            for (int64_t p = 0; p < k; ++p) {
                for (int64_t q = 0; q < k; ++q) {
                    double d = 0.0;
                    for (int dd = 0; dd < 3; ++dd) {
                        const double t = c[3 * size_t(q) + dd] - c[3 * size_t(p) + dd];
                        d += t * t;
                    }
                    d2c[size_t(q)] = d;
                    order[size_t(q)] = int32_t(q);
                }
                std::partial_sort(order.begin(), order.begin() + nc, order.end(), [&](int32_t a, int32_t b) {
                    return d2c[size_t(a)] != d2c[size_t(b)] ? d2c[size_t(a)] < d2c[size_t(b)] : a < b;
                });
                std::copy(order.begin(), order.begin() + nc, cand.begin() + size_t(p) * kCandidates);
            }
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t p = part[size_t(e)];
                next[size_t(e)] = p;
                // (after the first iterations the cells only shift: a tet whose face neighbours all share its cell stays)
                if (it >= kLloydFull && in_cell(int32_t(e), p) == faces(int32_t(e))) continue;
                int32_t best = p;
                double best_d = std::numeric_limits<double>::max();
                for (int j = 0; j < nc; ++j) {
                    const int32_t q = cand[size_t(p) * kCandidates + size_t(j)];
                    double d = -w[size_t(q)];
                    for (int dd = 0; dd < 3; ++dd) {
                        const double t = x[3 * size_t(e) + dd] - c[3 * size_t(q) + dd];
                        d += t * t;
                    }
                    if (d < best_d || (d == best_d && q < best)) {
                        best_d = d;
                        best = q;
                    }
                }
                next[size_t(e)] = best;
            }
            part.swap(next);
        }
    }

    // ---- 3. every cell keeps its largest face-connected piece; the others join neighbouring cells ----
    void connect()
    {
        std::vector<int32_t> piece(size_t(cnt), -1), best_piece(size_t(k), -1);
        std::vector<int64_t> piece_size;
        for (int64_t s0 = 0; s0 < cnt; ++s0) {
            if (piece[size_t(s0)] >= 0) continue;
            const int32_t id = int32_t(piece_size.size()), p = part[size_t(s0)];
            queue.assign(1, int32_t(s0));
            piece[size_t(s0)] = id;
            for (size_t h = 0; h < queue.size(); ++h)
                for (int f = 0; f < 4; ++f) {
                    const int32_t r = nb[4 * size_t(queue[h]) + f];
                    if (r < 0 || piece[size_t(r)] >= 0 || part[size_t(r)] != p) continue;
                    piece[size_t(r)] = id;
                    queue.push_back(r);
                }
            piece_size.push_back(int64_t(queue.size()));
            if (best_piece[size_t(p)] < 0 || piece_size[size_t(best_piece[size_t(p)])] < int64_t(queue.size())) best_piece[size_t(p)] = id;
        }
        int64_t left = 0;
        for (int64_t e = 0; e < cnt; ++e)
            if (piece[size_t(e)] != best_piece[size_t(part[size_t(e)])]) {
                part[size_t(e)] = -1;
                ++left;
            }
        while (left > 0) {   // (the sphere is face-connected: every sweep settles at least one tet)
            for (int64_t e = 0; e < cnt; ++e) {
                if (part[size_t(e)] >= 0) continue;
                int32_t pc[4], nn[4];
                int np = 0;
                for (int f = 0; f < 4; ++f) {
                    const int32_t r = nb[4 * size_t(e) + f];
                    if (r < 0 || part[size_t(r)] < 0) continue;
                    const int32_t pr = part[size_t(r)];
                    int j = int(std::find(pc, pc + np, pr) - pc);
                    if (j == np) {
                        pc[np] = pr;
                        nn[np++] = 0;
                    }
                    ++nn[j];
                }
                if (np == 0) continue;
                int j = 0;
                for (int i = 1; i < np; ++i)
                    if (nn[i] > nn[j] || (nn[i] == nn[j] && pc[i] < pc[j])) j = i;
                part[size_t(e)] = pc[j];
                --left;
            }
        }
    }

    // ---- exact slot / tile-vertex bookkeeping ----
    void add_slot(int32_t p, int32_t e)
    {
        ++slots[size_t(p)];
        for (int a = 0; a < 4; ++a) {
            int32_t &c = inc[size_t(p) * size_t(nv) + size_t(lv[4 * size_t(e) + a])];
            if (c % kMaxRank == 0) ++verts[size_t(p)];
            ++c;
        }
    }
    void remove_slot(int32_t p, int32_t e)
    {
        --slots[size_t(p)];
        for (int a = 0; a < 4; ++a) {
            int32_t &c = inc[size_t(p) * size_t(nv) + size_t(lv[4 * size_t(e) + a])];
            --c;
            if (c % kMaxRank == 0) --verts[size_t(p)];
        }
    }
    void build_state()
    {
        owned.assign(size_t(k), 0);
        slots.assign(size_t(k), 0);
        verts.assign(size_t(k), 0);
        inc.assign(size_t(k) * size_t(nv), 0);
        for (int64_t q = 0; q < cnt; ++q) {
            const int32_t pq = part[size_t(q)];
            ++owned[size_t(pq)];
            add_slot(pq, int32_t(q));
            int32_t seen[4];
            int ns = 0;
            for (int f = 0; f < 4; ++f) {
                const int32_t r = nb[4 * size_t(q) + f];
                if (r < 0) continue;
                const int32_t pr = part[size_t(r)];
                if (pr == pq || std::find(seen, seen + ns, pr) != seen + ns) continue;
                seen[ns++] = pr;
                add_slot(pr, int32_t(q));
            }
        }
    }
    int in_cell(int32_t q, int32_t p) const   // face neighbours of q in cell p
    {
        int n = 0;
        for (int f = 0; f < 4; ++f) {
            const int32_t r = nb[4 * size_t(q) + f];
            n += r >= 0 && part[size_t(r)] == p;
        }
        return n;
    }
    int faces(int32_t q) const   // face neighbours of q
    {
        int n = 0;
        for (int f = 0; f < 4; ++f) n += nb[4 * size_t(q) + f] >= 0;
        return n;
    }
    bool first_of(int32_t e, int f) const   // face f of e is the first one to name its neighbour
    {
        for (int g = 0; g < f; ++g)
            if (nb[4 * size_t(e) + g] == nb[4 * size_t(e) + f]) return false;
        return true;
    }
    // Moving e from its cell A to cell B: the tets that leave A's slots (e itself when no face neighbour stays in A, and halo
    // tets that were there for e alone) and those that join B's halo (neighbours of e that B did not reach yet).
    int leaving(int32_t e, int32_t A, int32_t *out) const
    {
        int n = 0;
        if (in_cell(e, A) == 0) out[n++] = e;
        for (int f = 0; f < 4; ++f) {
            const int32_t q = nb[4 * size_t(e) + f];
            if (q < 0 || part[size_t(q)] == A || !first_of(e, f)) continue;
            if (in_cell(q, A) == 1) out[n++] = q;
        }
        return n;
    }
    int entering(int32_t e, int32_t B, int32_t *out) const
    {
        int n = 0;
        for (int f = 0; f < 4; ++f) {
            const int32_t q = nb[4 * size_t(e) + f];
            if (q < 0 || part[size_t(q)] == B || !first_of(e, f)) continue;
            if (in_cell(q, B) == 0) out[n++] = q;
        }
        return n;
    }
    // change of cell p's tile vertices when the n tets t[] join (sign +1) or leave (-1) its slots
    int64_t vert_delta(int32_t p, const int32_t *t, int n, int sign) const
    {
        int32_t vs[20], ds[20];
        int m = 0;
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 4; ++a) {
                const int32_t v = lv[4 * size_t(t[i]) + a];
                int j = int(std::find(vs, vs + m, v) - vs);
                if (j == m) {
                    vs[m] = v;
                    ds[m++] = 0;
                }
                ds[j] += sign;
            }
        int64_t d = 0;
        for (int j = 0; j < m; ++j) {
            const int32_t c = inc[size_t(p) * size_t(nv) + size_t(vs[j])];
            d += copies(c + ds[j]) - copies(c);
        }
        return d;
    }
    struct Move {
        int32_t e = -1, B = -1;
        int64_t dcost = 0, key = 0;
        int nl = 0, ne = 0;
        int32_t gone[5], en[4];
        int64_t dsA = 0, dvA = 0, dsB = 0, dvB = 0;
    };
    // evaluates moving e to B; false if B would not fit
    bool evaluate(int32_t e, int32_t B, Move &mv) const
    {
        const int32_t A = part[size_t(e)];
        mv.e = e;
        mv.B = B;
        mv.nl = leaving(e, A, mv.gone);
        mv.ne = entering(e, B, mv.en);
        mv.dsA = -mv.nl;
        mv.dsB = mv.ne;
        mv.dvB = vert_delta(B, mv.en, mv.ne, +1);
        if (!lim.fits(slots[size_t(B)] + mv.dsB, verts[size_t(B)] + mv.dvB)) return false;
        mv.dvA = vert_delta(A, mv.gone, mv.nl, -1);
        mv.dcost = kPartSlotWeight * (mv.dsA + mv.dsB) + mv.dvA + mv.dvB;
        return true;
    }
    void apply(const Move &mv)
    {
        const int32_t A = part[size_t(mv.e)];
        for (int i = 0; i < mv.nl; ++i) remove_slot(A, mv.gone[i]);
        for (int i = 0; i < mv.ne; ++i) add_slot(mv.B, mv.en[i]);
        part[size_t(mv.e)] = mv.B;
        --owned[size_t(A)];
        ++owned[size_t(mv.B)];
    }
    // does cell A stay face-connected without e?  (a bounded search: a probe that runs out of budget refuses the move)
    bool stays_connected(int32_t e)
    {
        const int32_t A = part[size_t(e)];
        int32_t want[4];
        int nw = 0;
        for (int f = 0; f < 4; ++f) {
            const int32_t q = nb[4 * size_t(e) + f];
            if (q >= 0 && part[size_t(q)] == A && std::find(want, want + nw, q) == want + nw) want[nw++] = q;
        }
        if (nw <= 1) return true;
        if (++stamp == std::numeric_limits<int32_t>::max()) {
            std::fill(mark.begin(), mark.end(), 0);
            stamp = 1;
        }
        mark[size_t(e)] = stamp;
        mark[size_t(want[0])] = stamp;
        queue.assign(1, want[0]);
        int found = 1;
        for (size_t h = 0; h < queue.size() && h < size_t(kConnectProbe); ++h)
            for (int f = 0; f < 4; ++f) {
                const int32_t r = nb[4 * size_t(queue[h]) + f];
                if (r < 0 || part[size_t(r)] != A || mark[size_t(r)] == stamp) continue;
                mark[size_t(r)] = stamp;
                if (std::find(want, want + nw, r) != want + nw && ++found == nw) return true;
                queue.push_back(r);
            }
        return false;
    }
    // cells across the faces of e other than its own
    int other_cells(int32_t e, int32_t *out) const
    {
        const int32_t A = part[size_t(e)];
        int n = 0;
        for (int f = 0; f < 4; ++f) {
            const int32_t q = nb[4 * size_t(e) + f];
            if (q < 0) continue;
            const int32_t pq = part[size_t(q)];
            if (pq != A && std::find(out, out + n, pq) == out + n) out[n++] = pq;
        }
        return n;
    }

    // ---- 4a. move tets out of every cell that does not fit, cheapest first, until it fits ----
    bool repair()
    {
        std::vector<int32_t> members;
        for (int64_t A = 0; A < k; ++A) {
            if (fits(A)) continue;
            members.clear();
            for (int64_t e = 0; e < cnt; ++e)
                if (part[size_t(e)] == A) members.push_back(int32_t(e));
            while (!fits(A)) {
                if (owned[size_t(A)] <= 1) return false;
                // key: the change of the total cost, with the cell's own shrinkage counted twice
                Move best, mv;
                bool have = false;
                for (int32_t e : members) {
                    if (part[size_t(e)] != A) continue;
                    int32_t oc[4];
                    const int no = other_cells(e, oc);
                    for (int j = 0; j < no; ++j) {
                        if (!evaluate(e, oc[j], mv)) continue;
                        mv.key = mv.dcost + kPartSlotWeight * mv.dsA + mv.dvA;
                        if (have && mv.key >= best.key) continue;
                        if (!stays_connected(e)) break;
                        best = mv;
                        have = true;
                    }
                }
                if (!have) return false;
                apply(best);
            }
        }
        return true;
    }

    // ---- 4b. greedy sweeps of the moves that lower the cost ----
    void improve()
    {
        for (int sweep = 0; sweep < kImproveSweeps; ++sweep) {
            int64_t moved = 0;
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t A = part[size_t(e)];
                if (owned[size_t(A)] <= 1) continue;
                int32_t oc[4];
                const int no = other_cells(int32_t(e), oc);
                Move best, mv;
                bool have = false;
                for (int j = 0; j < no; ++j) {
                    if (!evaluate(int32_t(e), oc[j], mv) || mv.dcost >= 0) continue;
                    if (have && mv.dcost >= best.dcost) continue;
                    best = mv;
                    have = true;
                }
                if (have && stays_connected(int32_t(e))) {
                    apply(best);
                    ++moved;
                }
            }
            if (moved == 0) break;
        }
    }
};

}  // namespace

bool partition_component(const Mesh &M, const Limits &lim, const float *cen, const int32_t *ids, int64_t cnt,
                         int64_t k_first, int64_t k_last, Scratch &S, std::vector<std::vector<int32_t>> &parts,
                         int64_t &cost)
{
    parts.clear();
    cost = 0;
    k_first = std::max<int64_t>(2, k_first);
    k_last = std::min(k_last, cnt);
    if (k_first > k_last) return false;
    Part P(lim);
    P.cnt = cnt;
    P.nb.resize(4 * size_t(cnt));
    P.lv.resize(4 * size_t(cnt));
    P.x.resize(3 * size_t(cnt));
    const int32_t st = S.next();
    for (int64_t i = 0; i < cnt; ++i) {
        S.tet_stamp[size_t(ids[i])] = st;
        S.tet_slot[size_t(ids[i])] = int32_t(i);
    }
    for (int64_t i = 0; i < cnt; ++i) {
        const int64_t g = ids[i];
        for (int f = 0; f < 4; ++f) {
            const int32_t q = M.nbr[4 * g + f];
            P.nb[4 * size_t(i) + f] = q >= 0 && S.tet_stamp[size_t(q)] == st ? S.tet_slot[size_t(q)] : -1;
            const int32_t v = M.tets[4 * g + f];
            if (S.vert_stamp[size_t(v)] != st) {
                S.vert_stamp[size_t(v)] = st;
                S.vert_local[size_t(v)] = int32_t(P.nv++);
            }
            P.lv[4 * size_t(i) + f] = S.vert_local[size_t(v)];
        }
        for (int d = 0; d < 3; ++d) P.x[3 * size_t(i) + d] = cen[3 * size_t(g) + d];
    }
    if (k_last * P.nv > kMaxIncidence) return false;   // (the caller keeps the bisection)
    P.mark.assign(size_t(cnt), 0);
    std::vector<int32_t> idx(static_cast<size_t>(cnt));
    for (int64_t k = k_first; k <= k_last; ++k) {
        P.k = k;
        P.part.assign(size_t(cnt), 0);
        for (int64_t i = 0; i < cnt; ++i) idx[size_t(i)] = int32_t(i);
        int32_t next = 0;
        P.seed(idx.data(), cnt, k, next);
        P.lloyd();
        P.connect();
        P.build_state();
        if (!P.repair()) continue;
        P.improve();
        std::vector<int64_t> at(size_t(k), -1);
        for (int64_t p = 0; p < k; ++p)
            if (P.owned[size_t(p)] > 0) {
                at[size_t(p)] = int64_t(parts.size());
                parts.emplace_back();
                parts.back().reserve(size_t(P.owned[size_t(p)]));
                cost += P.cost(p);
            }
        for (int64_t i = 0; i < cnt; ++i) parts[size_t(at[size_t(P.part[size_t(i)])])].push_back(ids[i]);
        return true;
    }
    return false;
}

}  // namespace tsamd
