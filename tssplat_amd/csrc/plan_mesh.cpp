// Planner stage "mesh": face adjacency, an explicit element operator as per-face weights, connected components (= tet-spheres)
// and rest centroids.  Pure C++17, no HIP.
#include "planner.h"

#include <cmath>

namespace tsamd {
namespace {

inline void sort3(uint32_t &a, uint32_t &b, uint32_t &c)
{
    if (a > b) std::swap(a, b);
    if (b > c) std::swap(b, c);
    if (a > b) std::swap(a, b);
}

struct BucketFace {
    uint32_t b, c, slot;  // the smallest vertex is the bucket id; slot = 4*tet + opposite local vertex
};

}  // namespace

// nbr[4e+k] = tet across the face of e opposite local vertex k, -1 on the boundary.
int build_adjacency(const int32_t *tets, int64_t n, int64_t m, std::vector<int32_t> &nbr, int nthreads,
                    std::string &err)
{
    static const int opp[4][3] = {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}};
    nbr.assign(size_t(4 * m), -1);
    // bucket the 4 m faces by their smallest vertex: count, prefix sum, fill -- counting and filling in parallel with
    // atomic per-bucket cursors (the order inside a bucket is arbitrary here; every bucket is sorted below)
    std::vector<std::atomic<int32_t>> count(static_cast<size_t>(n));
    parallel_chunks(n, 1 << 16, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t v = b; v < e; ++v) count[size_t(v)].store(0, std::memory_order_relaxed);
    });
    parallel_chunks(m, 1 << 15, nthreads, [&](int64_t eb, int64_t ee, int) {
        for (int64_t e = eb; e < ee; ++e) {
            const int32_t *t = tets + 4 * e;
            for (int k = 0; k < 4; ++k) {
                uint32_t a = t[opp[k][0]], b = t[opp[k][1]], c = t[opp[k][2]];
                sort3(a, b, c);
                count[a].fetch_add(1, std::memory_order_relaxed);
            }
        }
    });
    std::vector<int64_t> start(size_t(n + 1), 0);
    for (int64_t v = 0; v < n; ++v) start[v + 1] = start[v] + count[size_t(v)].load(std::memory_order_relaxed);
    RawVector<BucketFace> faces(size_t(4 * m));
    parallel_chunks(n, 1 << 16, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t v = b; v < e; ++v) count[size_t(v)].store(0, std::memory_order_relaxed);
    });
    parallel_chunks(m, 1 << 15, nthreads, [&](int64_t eb, int64_t ee, int) {
        for (int64_t e = eb; e < ee; ++e) {
            const int32_t *t = tets + 4 * e;
            for (int k = 0; k < 4; ++k) {
                uint32_t a = t[opp[k][0]], b = t[opp[k][1]], c = t[opp[k][2]];
                sort3(a, b, c);
                const int64_t pos = start[a] + count[a].fetch_add(1, std::memory_order_relaxed);
                faces[size_t(pos)] = BucketFace{b, c, uint32_t(4 * e + k)};
            }
        }
    });
    std::atomic<int> bad{0};
    parallel_chunks(n, 4096, nthreads, [&](int64_t vb, int64_t ve, int) {
        for (int64_t v = vb; v < ve; ++v) {
            BucketFace *f0 = faces.data() + start[v], *f1 = faces.data() + start[v + 1];
            std::sort(f0, f1, [](const BucketFace &x, const BucketFace &y) {
                return x.b != y.b ? x.b < y.b : (x.c != y.c ? x.c < y.c : x.slot < y.slot);
            });
            for (BucketFace *f = f0; f + 1 < f1; ++f) {
                if (f->b == f[1].b && f->c == f[1].c) {
                    if (f + 2 < f1 && f[2].b == f->b && f[2].c == f->c) {
                        bad.store(1);
                        return;
                    }
                    nbr[f->slot] = int32_t(f[1].slot >> 2);
                    nbr[f[1].slot] = int32_t(f->slot >> 2);
                    ++f;
                }
            }
        }
    });
    if (bad.load()) {
        err = "non-manifold tet mesh: a face is shared by more than two tets";
        return ERR_BAD_MESH;
    }
    return OK;
}

// ---- explicit element operator: CSR -> (diagonal, one weight per tet face) ----
int operator_face_weights(const ElementOperatorCSR &op, const int32_t *nbr, int64_t m, bool rebuild_requested,
                          std::vector<float> &diag, std::vector<float> &w, bool &symmetric, std::string &err)
{
    if (!op.rowptr || (m > 0 && op.rowptr[m] > 0 && (!op.col || !op.val))) {
        err = "element operator: null CSR array";
        return ERR_INVALID;
    }
    if (op.rowptr[0] != 0 || op.rowptr[m] < 0) {
        err = "element operator: rowptr[0] must be 0 and rowptr[m] non-negative";
        return ERR_INVALID;
    }
    if (rebuild_requested) {
        err = "element operator: not combined with rebuild_dminv (the explicit-operator kernels stream Dm^-1)";
        return ERR_INVALID;
    }
    diag.assign(size_t(m), 0.f);
    w.assign(size_t(4 * m), 0.f);
    std::vector<double> dg(static_cast<size_t>(m), 0.0), wd(static_cast<size_t>(4 * m), 0.0);
    for (int64_t e = 0; e < m; ++e) {
        if (op.rowptr[e + 1] < op.rowptr[e]) {
            err = "element operator: rowptr is not monotone";
            return ERR_INVALID;
        }
        for (int64_t q = op.rowptr[e]; q < op.rowptr[e + 1]; ++q) {
            const int64_t j = op.col[q];
            const double v = op.val[q];
            if (!std::isfinite(v)) {
                err = "element operator: non-finite value in row " + std::to_string(e);
                return ERR_INVALID;
            }
            if (j == e) {
                dg[size_t(e)] += v;
                continue;
            }
            int k = -1;
            for (int f = 0; f < 4; ++f)
                if (j >= 0 && nbr[4 * size_t(e) + f] == j) {
                    k = f;
                    break;
                }
            if (k >= 0) {
                wd[4 * size_t(e) + k] += v;
            } else if (v != 0.0) {
                err = "element operator: entry (" + std::to_string(e) + ", " + std::to_string(j) +
                      ") is neither on the diagonal nor a face adjacency of the mesh";
                return ERR_INVALID;
            }
        }
    }
    for (int64_t e = 0; e < m; ++e) diag[size_t(e)] = float(dg[size_t(e)]);   // double -> fp32, as the
    for (int64_t i = 0; i < 4 * m; ++i) w[size_t(i)] = float(wd[size_t(i)]);  // reference rounds its matrices
    // symmetric in fp32?  then the column weights are the row weights and their four planes are not stored (kPlanesWeightedSym)
    symmetric = true;
    for (int64_t e = 0; e < m && symmetric; ++e)
        for (int k = 0; k < 4; ++k) {
            const int32_t q = nbr[4 * size_t(e) + k];
            if (q < 0) continue;
            float back = 0.f;
            for (int f = 0; f < 4; ++f)
                if (nbr[4 * size_t(q) + f] == e) back = w[4 * size_t(q) + f];
            if (back != w[4 * size_t(e) + k]) {
                symmetric = false;
                break;
            }
        }
    return OK;
}

// ---- connected components over face adjacency (each tet-sphere is one) ----
// Lock-free union-find over the face adjacency: the larger root is always linked under the smaller one, so a
// component's root is its smallest tet id whatever the thread interleaving -- components are then numbered by that
// id and list their tets in increasing order, exactly what a serial flood fill produces.
Components connected_components(const int32_t *nbr, int64_t m, int nthreads)
{
    std::vector<std::atomic<int32_t>> parent(static_cast<size_t>(m));
    parallel_chunks(m, 1 << 16, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; ++i) parent[size_t(i)].store(int32_t(i), std::memory_order_relaxed);
    });
    auto find = [&](int32_t x) {
        for (;;) {
            const int32_t p = parent[size_t(x)].load(std::memory_order_relaxed);
            if (p == x) return x;
            const int32_t gp = parent[size_t(p)].load(std::memory_order_relaxed);
            if (gp != p) {   // path halving (a lost race only skips the shortcut)
                int32_t expect = p;
                parent[size_t(x)].compare_exchange_weak(expect, gp, std::memory_order_relaxed);
            }
            x = p;
        }
    };
    parallel_chunks(m, 1 << 15, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; ++i)
            for (int k = 0; k < 4; ++k) {
                const int32_t q = nbr[4 * size_t(i) + k];
                if (q < 0 || q > i) continue;            // every interior face once, from its larger tet
                int32_t ra = find(int32_t(i)), rb = find(q);
                while (ra != rb) {
                    int32_t hi = std::max(ra, rb), lo = std::min(ra, rb);
                    int32_t expect = hi;
                    if (parent[size_t(hi)].compare_exchange_strong(expect, lo, std::memory_order_relaxed)) break;
                    ra = find(hi);
                    rb = find(lo);
                }
            }
    });
    // roots in increasing order = component numbers; tets of a component in increasing order (counting sort)
    std::vector<int32_t> root_comp(static_cast<size_t>(m), -1);
    RawVector<int32_t> root_of(static_cast<size_t>(m));
    parallel_chunks(m, 1 << 15, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; ++i) root_of[size_t(i)] = find(int32_t(i));
    });
    int64_t ncomp = 0;
    for (int64_t i = 0; i < m; ++i)
        if (root_of[size_t(i)] == i) root_comp[size_t(i)] = int32_t(ncomp++);
    Components out;
    out.tets.resize(size_t(m));
    std::vector<int64_t> fill(static_cast<size_t>(ncomp) + 1, 0);
    RawVector<int32_t> comp(static_cast<size_t>(m));   // tet -> component
    for (int64_t i = 0; i < m; ++i) {
        comp[size_t(i)] = root_comp[size_t(root_of[size_t(i)])];
        ++fill[size_t(comp[size_t(i)]) + 1];
    }
    for (int64_t c = 0; c < ncomp; ++c) fill[size_t(c) + 1] += fill[size_t(c)];
    out.start.assign(fill.begin(), fill.end());
    for (int64_t i = 0; i < m; ++i) out.tets[size_t(fill[size_t(comp[size_t(i)])]++)] = int32_t(i);
    return out;
}

// ---- tet centroids (rest state) ----
std::vector<float> tet_centroids(const Mesh &M, int nthreads)
{
    std::vector<float> cen(static_cast<size_t>(3 * M.m));
    parallel_chunks(M.m, 1 << 16, nthreads, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; ++i)
            for (int d = 0; d < 3; ++d) {
                float s = 0.f;
                for (int a = 0; a < 4; ++a) s += M.rest[3 * size_t(M.tets[4 * i + a]) + d];
                cen[3 * size_t(i) + d] = 0.25f * s;
            }
    });
    return cen;
}

}  // namespace tsamd
