// Multiresolution hash-grid encoding (Instant-NGP; tiny-cuda-nn's `Grid` encoding, 3-D, trilinear): the colour field of the
// texture stage (materials/explicit_material.py, models/networks.py:97-106).  Semantics: tests/hashgrid_oracle.py.
#pragma once

#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>

namespace tsamd {

constexpr int kGridMaxLevels = 32;
// dL/dparams of a level is accumulated in LDS when its table (entries x F x 4 bytes) fits this (gfx950: 160 KB per CU)
constexpr int kGridLdsBytes = 128 * 1024;

// Host-computed per-level table, passed to the kernels by value.
struct GridLevels {
    int64_t offset[kGridMaxLevels];      // first entry of the level (entries, not floats)
    uint32_t entries[kGridMaxLevels];    // the level's entry count (the `% hashmap_size` of grid_index)
    uint32_t res[kGridMaxLevels];
    float scale[kGridMaxLevels];
    uint32_t hashed[kGridMaxLevels];     // 1: coherent prime hash, 0: dense stride index
    int32_t n_levels;
    int32_t lds_levels;                  // levels [0, lds_levels) accumulate dL/dparams in LDS (their table fits)
};

// Fills `lv` (lds_levels = 0) and the total parameter count; false + `err` on a config the encoding does not accept.
bool grid_layout(int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                 int32_t dense, GridLevels &lv, int64_t &n_params, std::string &err);

hipError_t launch_grid_encode(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features, float *out,
                              hipStream_t stream);
hipError_t launch_grid_encode_backward(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                       const float *grad_out, float *grad_params, float *grad_x, hipStream_t stream);

// The sorted route to dL/dparams: no float atomics.  Contract:
//  * Repeatability: for given x, grad_out, config and initial contents of grad_params the resulting grad_params is ONE bit
//    pattern -- across repeated calls, on any stream, whatever else the device runs, whatever the workspace held on entry and
//    wherever it lies.  Every entry's adds are summed in an order fixed by (n, config) and the points' order; the result is not
//    promised to be invariant under a permutation of the points.
//  * Accuracy: |g - ref| <= 2e-5 * sum|adds| + 1e-6 against the float64 oracle (tests/hashgrid_oracle.py::encode_backward), the
//    bound of the atomic route; fp32 sums of 512-record chunks added in chunk order stay orders of magnitude inside it.
//  * Like the atomic route it ADDS into grad_params (zero it first).  dL/dx is the atomic route's kernel, bit for bit.
//  * Points go through in chunks of kGridSortedChunk, in order, on the caller's stream; the workspace is bounded by one chunk.
//    No allocation, no host synchronisation; all launch geometry is a function of (n, config).
constexpr int64_t kGridSortedChunk = int64_t(1) << 20;     // points per chunk (8 records each)
constexpr int kGridSortTile = 4096;                        // records per workgroup of a radix pass
constexpr int kGridSumRun = 512;                           // records per wave of the segmented sum
constexpr int64_t kGridWorkspaceAlign = 256;

inline int64_t grid_align_up(int64_t bytes) { return (bytes + kGridWorkspaceAlign - 1) / kGridWorkspaceAlign * kGridWorkspaceAlign; }

// Of n points still to go, the next chunk's points (at most kGridSortedChunk), its records, sort tiles and sum waves.
struct GridChunk {
    int64_t points, records, tiles, waves;
};

inline GridChunk grid_chunk(int64_t n)
{
    const int64_t nc = n < 0 ? 0 : (n < kGridSortedChunk ? n : kGridSortedChunk), n_rec = nc * 8;
    return {nc, n_rec, (n_rec + kGridSortTile - 1) / kGridSortTile, (n_rec + kGridSumRun - 1) / kGridSumRun};
}

// Byte offsets of the workspace's parts (each kGridWorkspaceAlign-aligned) and its size: a function of min(n, chunk) and F.
struct GridSortedWorkspace {
    int64_t rec_a, rec_b;      // 8-byte records (entry << 32 | 8 * point + corner), ping and pong
    int64_t gl;                // the level's grad_out slice, [points, F] f32
    int64_t hist, tot;         // [256][tiles] digit counts of a radix pass, and the 256 digit totals
    int64_t pkey, psum;        // boundary partials of the segmented sum: [2 * waves] keys, [2 * waves, F] sums
    int64_t bytes;
};

inline GridSortedWorkspace grid_sorted_workspace(int64_t n, int32_t n_features)
{
    const GridChunk c = grid_chunk(n);
    GridSortedWorkspace ws{};                      // (rec_a = 0)
    ws.rec_b = ws.rec_a + grid_align_up(c.records * 8);
    ws.gl = ws.rec_b + grid_align_up(c.records * 8);
    ws.hist = ws.gl + grid_align_up(c.points * n_features * 4);
    ws.tot = ws.hist + grid_align_up(256 * c.tiles * 4);
    ws.pkey = ws.tot + grid_align_up(256 * 4);
    ws.psum = ws.pkey + grid_align_up(2 * c.waves * 4);
    ws.bytes = c.points > 0 ? ws.psum + grid_align_up(2 * c.waves * n_features * 4) : 0;
    return ws;
}

hipError_t launch_grid_encode_backward_sorted(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                              const float *grad_out, float *grad_params, float *grad_x, void *workspace, hipStream_t stream);

// The planned route to dL/dparams: the sorted route with the sort taken out of the step.  A point plan is built once for a
// frozen point set (x, n, config): per chunk and level it keeps the low word `src = 8 * point_in_chunk + corner` of every
// sorted record, [chunk][level][8 * points_in_chunk] uint32 -- grid_plan_bytes(n, n_levels) bytes.  A planned backward is the
// sorted route's segmented sum over that stored order (one device body for both; the entry of a record is rebuilt from the
// point's cell, which the corner weight needs anyway) and its fold, every level of a chunk in one launch.  Contract:
//  1. Same bits as the sorted route: for the same x, grad_out, config and initial grad_params, grad_params ends bitwise equal
//     to launch_grid_encode_backward_sorted's.  Records, chunks, 512-record wave ranges, in-wave trees, carries and fold order
//     are the same, so the sorted route's accuracy bound and repeatability clause carry over unchanged.
//  2. The result does not depend on where the plan lies, nor on the planned workspace's contents or place; nothing is written
//     outside the plan (build) and grad_params + workspace (backward).
//  3. Memory safety: ANY byte pattern in the plan keeps every access in bounds.  A record is followed only while
//     src < 8 * points_in_chunk, which bounds the point index; its entry is computed from x, so it is always < entries.  A stale
//     or foreign plan gives wrong numbers, never an out-of-bounds access.
//  4. Build and backward make no allocation and no host synchronisation; all launch geometry is a function of (n, config).
// x, n and the config of a backward must be those the plan was built with.  It ADDS into grad_params.  There is no dL/dx with a
// plan: a planned point set is frozen by definition.
inline int64_t grid_plan_bytes(int64_t n, int32_t n_levels) { return grid_align_up((n < 0 ? 0 : n) * 8 * n_levels * 4); }

// The planned backward's workspace: the boundary partials of every level of one chunk, [level][2 * waves].
struct GridPlannedWorkspace {
    int64_t pkey, psum;        // [level][2 * waves] keys, [level][2 * waves, F] sums
    int64_t bytes;
};

inline GridPlannedWorkspace grid_planned_workspace(int64_t n, int32_t n_features, int32_t n_levels)
{
    const GridChunk c = grid_chunk(n);
    GridPlannedWorkspace ws{};                     // (pkey = 0)
    ws.psum = grid_align_up(n_levels * 2 * c.waves * 4);
    ws.bytes = c.points > 0 ? ws.psum + grid_align_up(n_levels * 2 * c.waves * n_features * 4) : 0;
    return ws;
}

// Build scratch: exactly grid_sorted_workspace(n, n_features).
hipError_t launch_grid_plan_build(const float *x, int64_t n, const GridLevels &lv, int32_t n_features, void *plan, void *workspace,
                                  hipStream_t stream);
hipError_t launch_grid_encode_backward_planned(const float *x, int64_t n, const GridLevels &lv, int32_t n_features, const float *grad_out,
                                               float *grad_params, const void *plan, void *workspace, hipStream_t stream);

}  // namespace tsamd
