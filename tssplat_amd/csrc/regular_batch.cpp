// Regular-batch detection (regular_batch.h): host code only.
#include "regular_batch.h"

namespace tsamd {

bool multiply_shift_for(uint32_t divisor, uint32_t n, uint32_t &mul, uint32_t &shift)
{
    mul = shift = 0;
    if (divisor == 0) return false;
    // ceil(2^s / d) is exact for every numerator below n once 2^s >= n d; smaller shifts may do as well, so take the first
    // that the index-by-index check accepts
    for (uint32_t s = 0; s < 63; ++s) {
        const uint64_t m = ((uint64_t(1) << s) + divisor - 1) / divisor;
        if (m >> 32) return false;
        bool ok = true;
        for (uint32_t t = 0; t < n && ok; ++t) ok = ((uint64_t(t) * m) >> s) == t / divisor;
        if (ok) {
            mul = uint32_t(m);
            shift = s;
            return true;
        }
    }
    return false;
}

namespace {

// tile t against tile 0: the same vertex count and every id moved by one positive constant (returned; 0 = no)
int64_t shift_against_tile0(const Plan &P, int64_t t)
{
    const TileDesc &a = P.tiles[0], &b = P.tiles[size_t(t)];
    if (a.n_verts != b.n_verts || a.n_verts <= 0) return 0;
    const int32_t *g0 = P.gvid.data() + a.vert_off, *gt = P.gvid.data() + b.vert_off;
    const int64_t V = int64_t(gt[0]) - int64_t(g0[0]);
    if (V <= 0) return 0;
    for (int32_t v = 1; v < a.n_verts; ++v)
        if (int64_t(gt[v]) - int64_t(g0[v]) != V) return 0;
    return V;
}

// the full comparison for period T and V vertices per copy; fills S and K
bool verify(const Plan &P, int64_t T, int64_t V, RegularBatch &out)
{
    const int64_t n_tiles = int64_t(P.tiles.size()), copies = n_tiles / T;
    const int64_t n_finish = int64_t(P.fin_vid.size());
    if (n_tiles % T != 0 || copies < 2 || n_finish % copies != 0 || P.n_stage % copies != 0) return false;
    if (int64_t(P.fin_off.size()) != n_finish + 1) return false;
    const int64_t K = n_finish / copies, S = P.n_stage / copies;
    if (V * (copies - 1) > INT32_MAX || S * copies > INT32_MAX) return false;
    for (int64_t t = T; t < n_tiles; ++t) {
        const int64_t r = t % T, c = t / T;
        const TileDesc &a = P.tiles[size_t(r)], &b = P.tiles[size_t(t)];
        if (a.n_verts != b.n_verts) return false;
        const int32_t *ga = P.gvid.data() + a.vert_off, *gb = P.gvid.data() + b.vert_off;
        const int32_t *da = P.vdst.data() + a.vert_off, *db = P.vdst.data() + b.vert_off;
        for (int32_t v = 0; v < a.n_verts; ++v) {
            if (int64_t(gb[v]) != int64_t(ga[v]) + c * V) return false;
            if (da[v] >= 0 ? int64_t(db[v]) != int64_t(da[v]) + c * V : (db[v] >= 0 || int64_t(~db[v]) != int64_t(~da[v]) + c * S)) return false;
        }
    }
    for (int64_t k = K; k < n_finish; ++k)
        if (int64_t(P.fin_vid[size_t(k)]) != int64_t(P.fin_vid[size_t(k % K)]) + (k / K) * V) return false;
    for (int64_t k = K; k <= n_finish; ++k)   // (the closing sentinel included: k % K == 0 there)
        if (K > 0 && int64_t(P.fin_off[size_t(k)]) != int64_t(P.fin_off[size_t(k % K)]) + (k / K) * S) return false;
    if (K == 0 && S != 0) return false;
    out.period = int32_t(T);
    out.copies = int32_t(copies);
    out.V = int32_t(V);
    out.S = int32_t(S);
    out.K = K;
    return true;
}

}  // namespace

RegularBatch detect_regular_batch(const Plan &P)
{
    const int64_t n_tiles = int64_t(P.tiles.size());
    if (n_tiles < 2 || n_tiles > INT32_MAX) return RegularBatch();
    for (int64_t T = 1; 2 * T <= n_tiles; ++T) {
        if (n_tiles % T != 0) continue;
        const int64_t V = shift_against_tile0(P, T);
        if (V == 0) continue;
        RegularBatch rb;
        if (!verify(P, T, V, rb)) continue;
        if (!multiply_shift_for(uint32_t(T), uint32_t(n_tiles), rb.div_mul, rb.div_shift)) return RegularBatch();
        return rb;
    }
    return RegularBatch();
}

}  // namespace tsamd
