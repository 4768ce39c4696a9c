// What the launch layer (eval_launch.cpp) and the kernels (tile_kernel.hip, step_kernels.hip) share and nobody else sees: the
// kernels' argument blocks and the handles -- function addresses and grids -- the launch layer reaches the kernels through.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "plan.h"

namespace tsamd {

struct KernelArgs {
    const TileDesc *tiles;
    const uint8_t *blob;
    const int32_t *gvid;
    const int32_t *vdst;  // per tile vertex: >= 0 row of grad, < 0 staging row ~vdst (plan.h)
    const float *x;
    const float *grad_out;
    float *grad;
    float *stage;
    double *partials;
    float c1, c2;
    float ratio;        // c2 / c1, divided on the host (set_coefficients): a division costs every wave of every tile a dozen instructions
    const float *coef;  // optional: (c1, c2) read on the device instead (tsamd_evaluate_dev_coef); the kernel then divides itself
    int order;
    int n_tiles;
    int tiles_per_xcd;
    int vert_stride;   // gvid / vdst entries per tile: tile t's vertex ids start at t * vert_stride (= its descriptor's vert_off)
    int n_planes;      // dword planes per slot (explicit-operator plans: 22, or 18 for a symmetric operator -- plan.h)
    // Regular batch (regular_batch.h): tile t is copy c = (t * reg_mul) >> reg_shift (64-bit product; = t / reg_period, checked on
    // the host for every tile) of template tile r = t - c * reg_period.  The first-round ids and destinations are read at r's
    // entries and corrected by c * reg_v vertices / c * reg_s staging rows.  All zero for any other plan: c = 0, r = t.
    uint32_t reg_period, reg_mul, reg_shift;
    int reg_v, reg_s;
};

struct FinishArgs {
    const int32_t *fin_vid, *fin_off;
    int64_t n_finish;
    const float *stage;
    float *grad;
    const float *grad_out;
    const double *partials;
    int64_t n_tiles;
    float c1, c2;
    const float *coef;  // optional device (c1, c2), see KernelArgs
    float *energy;
    double *terms;
    float *energy_copy;   // optional second destination of the energy (a replay's per-launch argument: the ring slot of an energy exchange)
    // Regular batch: reg_k > 0 finish entries per copy, n_finish = reg_copies * reg_k.  A thread owns template entry kk < reg_k and
    // walks copies c = blockIdx.y, blockIdx.y + gridDim.y, ...: entry c * reg_k + kk sums the template's rows moved by c * reg_s
    // into the template's vertex moved by c * reg_v.  reg_k == 0: every thread reads its own entries of the lists.
    int64_t reg_k;
    int reg_copies, reg_v, reg_s;
};

// ---- tile_kernel.hip ----
// One row per lane layout and operator variant the tile kernel is instantiated for; fn = {forward only, with gradient}.
struct TileKernelRow {
    int spt, cap;   // slots per lane, block-size cap
    bool weighted, rebuild;
    bool index_nt;  // false: the cache-retaining twin (tile_shared_index_kernel), for plans that share index planes
    const void *fn[2];
};
extern const TileKernelRow kTileKernels[9];
// index_nt: the plan shares (almost) no index planes (EvalArgs::index_nt); false selects the cache-retaining twin where one is built
const void *tile_kernel_for(int spt, int block_threads, bool grad, bool weighted, bool rebuild, bool index_nt);

// ---- step_kernels.hip ----
struct StepKernels {
    const void *finish, *energy_reduce;      // (FinishArgs): 256 threads, finish_grid() workgroups; 1 024 threads, one workgroup
    const void *adam_moments, *adam_apply;   // 256 threads, adam_grid() workgroups
};
StepKernels step_kernels();
unsigned finish_grid(int64_t n_finish);
dim3 finish_grid_regular(int64_t per_copy, int copies);   // FinishArgs::reg_k > 0
unsigned adam_grid(int64_t n);

}  // namespace tsamd
