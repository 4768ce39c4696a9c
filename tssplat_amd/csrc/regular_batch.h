// Regular batches (host side, no HIP in this header): a plan whose tiles, vertex ids, destinations and finish lists repeat with
// a period -- every copy of one template carries the template's per-vertex bookkeeping plus a constant.  The kernels then
// address the TEMPLATE's gvid / vdst / fin_vid / fin_off entries (bytes every copy shares: one template's lists stay in the XCD's L2,
// like the shared index planes) and add the copy's constant in registers.
#pragma once

#include <cstdint>

#include "plan.h"

namespace tsamd {

// Tile t = copy c = t / period of template tile r = t % period; V vertices, S staging rows and K finish entries per copy:
//   gvid[t][v]   == gvid[r][v] + c V                             for v < n_verts (tile t's n_verts == tile r's)
//   vdst[t][v]   == vdst[r][v] + c V  where vdst[r][v] >= 0,     ~vdst[t][v] == ~vdst[r][v] + c S  where it is negative
//   fin_vid[k]   == fin_vid[k % K] + (k / K) V,                  fin_off[k] == fin_off[k % K] + (k / K) S  (k = n_finish included)
// period == 0: the plan is not regular (or has a single copy) and everything else is 0.
struct RegularBatch {
    int32_t period = 0;
    int32_t copies = 0;
    int32_t V = 0, S = 0;
    int64_t K = 0;
    // t / period == (uint64_t(t) * div_mul) >> div_shift for every tile index t of the plan (checked for each of them); 0, 0
    // with period 0: the quotient is 0 and the remainder the tile itself
    uint32_t div_mul = 0, div_shift = 0;
};

// quotient and remainder of a tile index the way the kernels form them
inline uint32_t regular_copy(const RegularBatch &rb, uint32_t tile) { return uint32_t((uint64_t(tile) * rb.div_mul) >> rb.div_shift); }
inline uint32_t regular_template(const RegularBatch &rb, uint32_t tile) { return tile - regular_copy(rb, tile) * uint32_t(rb.period); }

// The multiply-shift pair of a divisor for numerators below n (the smallest shift whose rounded-up reciprocal is exact on
// [0, n), verified index by index); false if there is none with a 32-bit multiplier.
bool multiply_shift_for(uint32_t divisor, uint32_t n, uint32_t &mul, uint32_t &shift);

// Candidates (a later tile that looks like tile 0 moved by a constant) are named cheaply; the full comparison of every tile
// vertex and every finish entry decides.  Any mismatch under every candidate gives period 0: nothing is "nearly regular".
RegularBatch detect_regular_batch(const Plan &plan);

}  // namespace tsamd
