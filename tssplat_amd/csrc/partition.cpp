// Partition of one tet-sphere that does not fit into a single tile.
//
// What a tile costs the energy kernels is its SLOTS -- the owned tets plus the one-ring face halo, each streamed (52 B) and run
// through pass 1, pass 3 and the scatter -- and its tile vertices, whose partial sums go through the staging rows when another
// tile meets the vertex too (plan.h).  Both grow with the surface between tiles, and the recursive coordinate bisection of
// build_plan cuts slabs with a lot of surface.  Here the sphere is cut into compact cells instead, for every k the caller allows:
//   1. seed k cells with the bisection of the rest centroids by tet count -- or, when step 4 cannot make those fit, with k
//      centroids spread by farthest-point sampling;
//   2. slot-balanced Lloyd iterations: every tet joins the cell of least |x - c|^2 - w among the centres nearest its own cell's,
//      and the weight w of a cell falls when it holds more slots than the mean (a power diagram);
//   3. every cell keeps its largest face-connected piece, the other pieces join the neighbouring cells;
//   4. boundary moves between face-adjacent cells: first out of every cell that does not fit until it fits, then
//      Fiduccia-Mattheyses passes over kPartSlotWeight * slots + kPartRowWeight * staged rows.  A pass takes the best move of any
//      unlocked tet from a queue ordered by (gain, tet id) -- also when that gain is zero or negative, which is what carries a cut
//      across the plateaus of a lattice --, locks the tet, and in the end rolls back to the cheapest prefix of its moves.  Every
//      move keeps both cells fitting and face-connected, so every prefix is a valid cut.
// Everything runs in one thread per sphere over local indices in a fixed order with ties broken by tet id, so the result does
// not depend on the number of host threads.  A cell's slot count and tile vertices (kMaxRank slots per tile vertex, as
// measure() counts them) and the staged rows of the whole cut are kept exact under every move through per-(cell, vertex) slot
// counts and per-vertex copy counts.
#include "planner.h"

#include <algorithm>
#include <cmath>
#include <set>
#include <utility>

namespace tsamd {
namespace {

constexpr int kLloydIters = 12;
constexpr int kLloydFull = 4;                // of which assign every tet (the others: tets on a cell boundary)
constexpr int kCandidates = 8;               // centres a tet looks at: the nearest ones to its own cell's centre
constexpr int kGrowRounds = 6;               // rounds of the balanced growth over the face adjacency
constexpr int kFmPasses = 8;                 // at most; the passes end with the first one that finds nothing
constexpr int kFmStall = 3000;               // moves a pass may go on past its cheapest prefix
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
    std::vector<int32_t> tot;     // nv: tile-vertex copies of the vertex over all cells
    int64_t rows = 0;             // staged rows of the cut: the copies of every vertex that has more than one
    std::vector<int32_t> mark, queue;
    int32_t stamp = 0;

    explicit Part(const Limits &l) : lim(l) {}

    static int64_t staged(int64_t c) { return c > 1 ? c : 0; }
    int64_t total_slots() const
    {
        int64_t s = 0;
        for (int64_t p = 0; p < k; ++p) s += slots[size_t(p)];
        return s;
    }
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

    // ---- 3b. balanced growth over the face adjacency ----
    // Every cell starts again from the tet nearest its centroid and claims tets breadth-first across faces, the cell that
    // holds the fewest tets always moving next.  The cells that come out are balls of the mesh's own face-adjacency metric, not
    // of the rest coordinates: where the mesh is a lattice their walls follow its planes, which is where a wall cuts the fewest
    // faces.  Cells are face-connected by construction.
    void grow(int rounds)
    {
        const size_t K = size_t(k);
        std::vector<double> c(3 * K);
        std::vector<int64_t> n_in(K);
        std::vector<int32_t> centre(K), claimed(static_cast<size_t>(cnt));
        std::vector<std::vector<int32_t>> fifo(K);
        std::vector<size_t> head(K);
        for (int it = 0; it < rounds; ++it) {
            std::fill(c.begin(), c.end(), 0.0);
            std::fill(n_in.begin(), n_in.end(), 0);
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t p = part[size_t(e)];
                ++n_in[size_t(p)];
                for (int d = 0; d < 3; ++d) c[3 * size_t(p) + d] += x[3 * size_t(e) + d];
            }
            std::vector<double> best(K, std::numeric_limits<double>::max());
            std::fill(centre.begin(), centre.end(), -1);
            for (int64_t e = 0; e < cnt; ++e) {
                const int32_t p = part[size_t(e)];
                double d2 = 0.0;
                for (int d = 0; d < 3; ++d) {
                    const double t = x[3 * size_t(e) + d] - c[3 * size_t(p) + d] / double(n_in[size_t(p)]);
                    d2 += t * t;
                }
                if (d2 < best[size_t(p)]) {
                    best[size_t(p)] = d2;
                    centre[size_t(p)] = int32_t(e);
                }
            }
            std::fill(claimed.begin(), claimed.end(), -1);
            std::fill(n_in.begin(), n_in.end(), 0);
            for (size_t p = 0; p < K; ++p) {
                fifo[p].clear();
                head[p] = 0;
                if (centre[p] >= 0) fifo[p].push_back(centre[p]);
            }
            for (int64_t left = cnt; left > 0;) {
                // the cell with the fewest tets that still has somewhere to go (ties: the lowest)
                int64_t p = -1;
                for (size_t q = 0; q < K; ++q) {
                    while (head[q] < fifo[q].size() && claimed[size_t(fifo[q][head[q]])] >= 0) ++head[q];
                    if (head[q] < fifo[q].size() && (p < 0 || n_in[q] < n_in[size_t(p)])) p = int64_t(q);
                }
                if (p < 0) break;   // (cannot happen on a face-connected component)
                const int32_t e = fifo[size_t(p)][head[size_t(p)]++];
                claimed[size_t(e)] = int32_t(p);
                ++n_in[size_t(p)];
                --left;
                for (int f = 0; f < 4; ++f) {
                    const int32_t r = nb[4 * size_t(e) + f];
                    if (r >= 0 && claimed[size_t(r)] < 0) fifo[size_t(p)].push_back(r);
                }
            }
            for (int64_t e = 0; e < cnt; ++e)
                if (claimed[size_t(e)] >= 0) part[size_t(e)] = claimed[size_t(e)];
        }
    }

    // ---- exact slot / tile-vertex bookkeeping ----
    void copy_changed(int32_t v, int d)
    {
        rows -= staged(tot[size_t(v)]);
        tot[size_t(v)] += d;
        rows += staged(tot[size_t(v)]);
    }
    void add_slot(int32_t p, int32_t e)
    {
        ++slots[size_t(p)];
        for (int a = 0; a < 4; ++a) {
            int32_t &c = inc[size_t(p) * size_t(nv) + size_t(lv[4 * size_t(e) + a])];
            if (c % kMaxRank == 0) {
                ++verts[size_t(p)];
                copy_changed(lv[4 * size_t(e) + a], +1);
            }
            ++c;
        }
    }
    void remove_slot(int32_t p, int32_t e)
    {
        --slots[size_t(p)];
        for (int a = 0; a < 4; ++a) {
            int32_t &c = inc[size_t(p) * size_t(nv) + size_t(lv[4 * size_t(e) + a])];
            --c;
            if (c % kMaxRank == 0) {
                --verts[size_t(p)];
                copy_changed(lv[4 * size_t(e) + a], -1);
            }
        }
    }
    void build_state()
    {
        owned.assign(size_t(k), 0);
        slots.assign(size_t(k), 0);
        verts.assign(size_t(k), 0);
        inc.assign(size_t(k) * size_t(nv), 0);
        tot.assign(size_t(nv), 0);
        rows = 0;
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
    struct Move {
        int32_t e = -1, B = -1;
        int64_t dcost = 0, key = 0;
        int nl = 0, ne = 0;
        int32_t gone[5], en[4];
        int64_t dsA = 0, dvA = 0, dsB = 0, dvB = 0;
    };
    // evaluates moving e to B: the change of both cells' slots and tile vertices and of the cut's cost; false if B would not
    // fit (`check` off: a move that only takes a recorded one back)
    bool evaluate(int32_t e, int32_t B, Move &mv, bool check = true) const
    {
        const int32_t A = part[size_t(e)];
        mv.e = e;
        mv.B = B;
        mv.nl = leaving(e, A, mv.gone);
        mv.ne = entering(e, B, mv.en);
        mv.dsA = -mv.nl;
        mv.dsB = mv.ne;
        // per vertex: slots that leave A and slots that join B
        int32_t vs[36], dA[36], dB[36];
        int m = 0;
        auto note = [&](int32_t t, int32_t *d, int sign) {
            for (int a = 0; a < 4; ++a) {
                const int32_t v = lv[4 * size_t(t) + a];
                int j = int(std::find(vs, vs + m, v) - vs);
                if (j == m) {
                    vs[m] = v;
                    dA[m] = dB[m] = 0;
                    ++m;
                }
                d[j] += sign;
            }
        };
        for (int i = 0; i < mv.nl; ++i) note(mv.gone[i], dA, -1);
        for (int i = 0; i < mv.ne; ++i) note(mv.en[i], dB, +1);
        mv.dvA = mv.dvB = 0;
        int64_t drows = 0;
        for (int j = 0; j < m; ++j) {
            const int32_t cA = inc[size_t(A) * size_t(nv) + size_t(vs[j])], cB = inc[size_t(B) * size_t(nv) + size_t(vs[j])];
            const int64_t a = copies(cA + dA[j]) - copies(cA), b = copies(cB + dB[j]) - copies(cB);
            mv.dvA += a;
            mv.dvB += b;
            const int64_t t = tot[size_t(vs[j])];
            drows += staged(t + a + b) - staged(t);
        }
        if (check && !lim.fits(slots[size_t(B)] + mv.dsB, verts[size_t(B)] + mv.dvB)) return false;
        mv.dcost = kPartSlotWeight * (mv.dsA + mv.dsB) + kPartRowWeight * drows;
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
                        mv.key = mv.dcost + kPartSlotWeight * mv.dsA + kPartRowWeight * mv.dvA;
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

    // ---- 4b. Fiduccia-Mattheyses passes ----
    // the cheapest move of e to a cell across one of its faces (ties: the lower cell); false if there is none that fits
    bool best_move(int32_t e, Move &best) const
    {
        if (owned[size_t(part[size_t(e)])] <= 1) return false;
        int32_t oc[4];
        const int no = other_cells(e, oc);
        Move mv;
        bool have = false;
        for (int j = 0; j < no; ++j) {
            if (!evaluate(e, oc[j], mv)) continue;
            if (have && (mv.dcost > best.dcost || (mv.dcost == best.dcost && mv.B > best.B))) continue;
            best = mv;
            have = true;
        }
        return have;
    }
    std::set<std::pair<int64_t, int32_t>> fm_queue;   // (cost change, tet): the best gain first, ties by tet id
    std::vector<int64_t> fm_key;                      // per tet: its cost change in the queue
    std::vector<uint8_t> fm_queued, fm_locked;
    void fm_drop(int32_t e)
    {
        if (!fm_queued[size_t(e)]) return;
        fm_queue.erase({fm_key[size_t(e)], e});
        fm_queued[size_t(e)] = 0;
    }
    void fm_refresh(int32_t e)
    {
        fm_drop(e);
        Move mv;
        if (fm_locked[size_t(e)] || !best_move(e, mv)) return;
        fm_key[size_t(e)] = mv.dcost;
        fm_queued[size_t(e)] = 1;
        fm_queue.insert({mv.dcost, e});
    }
    // One pass; true if it lowered the cost.  The queue holds every unlocked tet's best move as it was last evaluated; a move is
    // evaluated again when it comes up and goes back into the queue if its gain is no longer what the queue said (the slot
    // counts of a vertex change under moves several tets away), so every move that is made is made at its exact gain.
    bool fm_pass()
    {
        fm_queue.clear();
        fm_key.assign(size_t(cnt), 0);
        fm_queued.assign(size_t(cnt), 0);
        fm_locked.assign(size_t(cnt), 0);
        for (int64_t e = 0; e < cnt; ++e) fm_refresh(int32_t(e));
        std::vector<std::pair<int32_t, int32_t>> done;   // (tet, the cell it came from)
        int64_t cum = 0, best = 0;
        size_t best_len = 0;
        while (!fm_queue.empty() && done.size() - best_len < size_t(kFmStall)) {
            const int32_t e = fm_queue.begin()->second;
            Move mv;
            if (!best_move(e, mv)) {
                fm_drop(e);
                continue;
            }
            if (mv.dcost != fm_key[size_t(e)]) {
                fm_queue.erase(fm_queue.begin());
                fm_key[size_t(e)] = mv.dcost;
                fm_queue.insert({mv.dcost, e});
                continue;
            }
            fm_drop(e);
            if (!stays_connected(e)) continue;   // (it comes back when a move next to it changes its cell)
            const int32_t A = part[size_t(e)];
            apply(mv);
            fm_locked[size_t(e)] = 1;
            done.push_back({e, A});
            cum += mv.dcost;
            if (cum < best) {
                best = cum;
                best_len = done.size();
            }
            // the moves within two faces of e have changed
            for (int f = 0; f < 4; ++f) {
                const int32_t q = nb[4 * size_t(e) + f];
                if (q < 0) continue;
                fm_refresh(q);
                for (int g = 0; g < 4; ++g) {
                    const int32_t r = nb[4 * size_t(q) + g];
                    if (r >= 0 && r != e) fm_refresh(r);
                }
            }
        }
        while (done.size() > best_len) {   // roll back to the cheapest prefix
            Move mv;
            evaluate(done.back().first, done.back().second, mv, false);
            apply(mv);
            done.pop_back();
        }
        return best < 0;
    }
    void improve()
    {
        for (int pass = 0; pass < kFmPasses; ++pass)
            if (!fm_pass()) break;
    }

    // ---- 1b. seeds spread by farthest-point sampling over the rest centroids; every tet joins the nearest one ----
    void seed_spread()
    {
        double mean[3] = {0.0, 0.0, 0.0};
        for (int64_t e = 0; e < cnt; ++e)
            for (int d = 0; d < 3; ++d) mean[d] += x[3 * size_t(e) + d];
        for (int d = 0; d < 3; ++d) mean[d] /= double(cnt);
        std::vector<double> d2(size_t(cnt), std::numeric_limits<double>::max());
        auto dist2 = [&](int64_t e, const double *c) {
            double s = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double t = x[3 * size_t(e) + d] - c[d];
                s += t * t;
            }
            return s;
        };
        int64_t far = 0;   // the first seed: the tet farthest from the mean (ties: the lowest id)
        double far_d = -1.0;
        for (int64_t e = 0; e < cnt; ++e) {
            const double d = dist2(e, mean);
            if (d > far_d) {
                far_d = d;
                far = e;
            }
        }
        for (int64_t p = 0; p < k; ++p) {
            const double *c = &x[3 * size_t(far)];
            int64_t next_far = 0;
            double next_d = -1.0;
            for (int64_t e = 0; e < cnt; ++e) {
                const double d = dist2(e, c);
                if (d < d2[size_t(e)]) {
                    d2[size_t(e)] = d;
                    part[size_t(e)] = int32_t(p);
                }
                if (d2[size_t(e)] > next_d) {
                    next_d = d2[size_t(e)];
                    next_far = e;
                }
            }
            far = next_far;
        }
    }
};

}  // namespace

bool partition_component(const Mesh &M, const Limits &lim, const float *cen, const int32_t *ids, int64_t cnt,
                         const std::vector<std::vector<int32_t>> &incumbent, int64_t k_first, int64_t k_last, int64_t slot_cap,
                         Scratch &S, std::vector<std::vector<int32_t>> &parts, CutStats &before, CutStats &after)
{
    parts.clear();
    before = after = CutStats();
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
    if (std::max<int64_t>(k_last, int64_t(incumbent.size())) * P.nv > kMaxIncidence) return false;   // (the caller keeps its cut)
    P.mark.assign(size_t(cnt), 0);
    // the incumbent's figures, counted the same way
    P.k = int64_t(incumbent.size());
    P.part.assign(size_t(cnt), 0);
    for (size_t p = 0; p < incumbent.size(); ++p)
        for (int32_t g : incumbent[p]) P.part[size_t(S.tet_slot[size_t(g)])] = int32_t(p);
    P.build_state();
    before.parts = P.k;
    before.slots = P.total_slots();
    before.rows = P.rows;
    std::vector<int32_t> idx(static_cast<size_t>(cnt)), best_part;
    int64_t best_k = 0;
    after = before;
    // one k: cells of the rest coordinates and cells grown over the face adjacency, each refined; true if either fitted
    auto try_k = [&](int64_t k) {
        P.k = k;
        bool any = false;
        for (int grown = 0; grown < 2; ++grown) {
            bool fitted = false;
            for (int spread = 0; spread < 2 && !fitted; ++spread) {
                P.part.assign(size_t(cnt), 0);
                if (spread) {
                    P.seed_spread();
                } else {
                    for (int64_t i = 0; i < cnt; ++i) idx[size_t(i)] = int32_t(i);
                    int32_t next = 0;
                    P.seed(idx.data(), cnt, k, next);
                }
                P.lloyd();
                P.connect();
                if (grown) P.grow(kGrowRounds);
                P.build_state();
                fitted = P.repair();
            }
            if (!fitted) continue;
            any = true;
            P.improve();
            CutStats now;
            for (int64_t p = 0; p < k; ++p) now.parts += P.owned[size_t(p)] > 0;
            now.slots = P.total_slots();
            now.rows = P.rows;
            if (now.cost() >= after.cost()) continue;
            after = now;
            best_part = P.part;
            best_k = k;
        }
        return any;
    };
    // upward from the caller's bound until two values of k have fitted (the cost rises with k from there on) ...
    int fitted_ks = 0;
    for (int64_t k = k_first; k <= k_last && fitted_ks < 2; ++k) fitted_ks += try_k(k) ? 1 : 0;
    // ... and downward while the best cut's own slots would go into fewer tiles than the caller's bound assumed
    for (int64_t k = k_first - 1; k >= 2 && best_k == k + 1 && (after.slots + slot_cap - 1) / slot_cap <= k; --k) try_k(k);
    if (best_k == 0 || after.cost() * kPartMinSavingDen > before.cost() * (kPartMinSavingDen - 1)) {
        after = before;
        return false;
    }
    std::vector<int64_t> at(size_t(best_k), -1);
    for (int64_t i = 0; i < cnt; ++i) {
        int64_t &a = at[size_t(best_part[size_t(i)])];
        if (a < 0) {
            a = int64_t(parts.size());
            parts.emplace_back();
        }
        parts[size_t(a)].push_back(ids[i]);
    }
    return true;
}

}  // namespace tsamd
