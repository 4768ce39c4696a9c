// The launch layer of the geometry energy: which kernels one evaluation launches with which arguments (LaunchRecipe), as stream
// launches, as a replayable HIP graph (EvalGraph) and as n optimisation steps in one graph (TrainLoopGraph).  Host code only: the
// kernels are const void * handles from tile_kernel.hip (kTileKernels, tile_kernel_for) and step_kernels.hip (step_kernels).
#include <vector>

#include "kernels.h"
#include "launch_args.h"

namespace tsamd {

bool lane_layout_supported(int spt, int max_threads) { return tile_kernel_for(spt, max_threads, true, false, false, true) != nullptr; }

hipError_t configure_kernels(int lds_bytes)
{
    // hipFuncAttributeMaxDynamicSharedMemorySize is per function, i.e. per process and device -- not per handle: only
    // ever raise it, or a handle with small tiles would lower the limit under an earlier handle with large ones
    static int configured[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (lds_bytes <= configured[dev]) return hipSuccess;
    // every tile kernel a plan can reach
    for (const TileKernelRow &row : kTileKernels)
        for (const void *fn : row.fn) {
            // lds_at() addresses the dynamic LDS array by absolute byte address: that is only right while the array starts
            // at LDS address 0, i.e. while the kernel has no static LDS object in front of it (a static __shared__ variable,
            // an LDS-using helper that was not inlined, a compiler-generated module-LDS block)
            hipFuncAttributes attr;
            hipError_t e = hipFuncGetAttributes(&attr, fn);
            if (e != hipSuccess) return e;
            if (attr.sharedSizeBytes != 0) return hipErrorInvalidDeviceFunction;
            e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
            if (e != hipSuccess) return e;
        }
    configured[dev] = lds_bytes;
    return hipSuccess;
}

namespace {

// What one evaluation launches: the tile kernel (if the plan has tiles) and then either the finish kernel (shared-vertex
// sums + the energy reduction in its workgroup 0) or, without a gradient, the energy reduction alone.  One description
// serves the stream launches below and the nodes of an EvalGraph.
struct LaunchRecipe {
    KernelArgs k;
    FinishArgs f;
    const void *tile_fn = nullptr, *finish_fn = nullptr;   // nullptr = not launched
    dim3 tile_grid, tile_block, finish_grid, finish_block;
    size_t tile_lds = 0;
};

void set_coefficients(KernelArgs &k, float c1, float c2)
{
    k.c1 = c1;
    k.c2 = c2;
    k.ratio = c2 / c1;   // (IEEE single-precision division, like the kernel's own: inf / NaN for c1 == 0 are handled there)
}

hipError_t make_recipe(const EvalArgs &e, LaunchRecipe &r)
{
    if (e.n_tiles > 0) {
        KernelArgs &k = r.k;
        k.tiles = e.tiles;
        k.blob = e.blob;
        k.gvid = e.gvid;
        k.vdst = e.vdst;
        k.x = e.x;
        k.grad_out = e.grad_out;
        k.grad = e.grad;
        k.stage = e.stage;
        k.partials = e.partials;
        set_coefficients(k, e.c1, e.c2);
        k.coef = e.coef;
        k.order = e.order;
        k.n_tiles = int(e.n_tiles);
        k.tiles_per_xcd = int((e.n_tiles + 7) / 8);
        k.vert_stride = e.vert_stride;
        k.n_planes = e.n_planes;
        k.reg_period = uint32_t(e.regular.period);   // (all five are 0 for a plan that is not regular)
        k.reg_mul = e.regular.div_mul;
        k.reg_shift = e.regular.div_shift;
        k.reg_v = e.regular.V;
        k.reg_s = e.regular.S;
        r.tile_fn = tile_kernel_for(e.spt, e.block_threads, e.grad != nullptr, e.weighted, e.rebuild, e.index_nt);
        if (!r.tile_fn) return hipErrorInvalidConfiguration;
        r.tile_block = dim3(unsigned(e.block_threads));
        r.tile_grid = dim3(unsigned(8 * k.tiles_per_xcd));
        r.tile_lds = size_t(e.lds_bytes);
    }
    FinishArgs &f = r.f;
    f.fin_vid = e.fin_vid;
    f.fin_off = e.fin_off;
    f.n_finish = e.grad ? e.n_finish : 0;
    f.stage = e.stage;
    f.grad = e.grad;
    f.grad_out = e.grad_out;
    f.partials = e.partials;
    f.n_tiles = e.n_tiles;
    f.c1 = e.c1;
    f.c2 = e.c2;
    f.coef = e.coef;
    f.energy = e.energy;
    f.terms = e.terms;
    f.energy_copy = nullptr;
    // (the x grid is capped: a copy with more entries than it covers -- no plan in sight -- takes the list loop)
    const bool regular = e.regular.period > 0 && e.regular.K > 0 && int64_t(finish_grid(e.regular.K) - 1) * 256 >= e.regular.K;
    f.reg_k = regular ? e.regular.K : 0;
    f.reg_copies = regular ? e.regular.copies : 0;
    f.reg_v = regular ? e.regular.V : 0;
    f.reg_s = regular ? e.regular.S : 0;
    if (f.n_finish > 0) {
        r.finish_fn = step_kernels().finish;
        r.finish_grid = regular ? finish_grid_regular(f.reg_k, f.reg_copies) : dim3(finish_grid(f.n_finish));
        r.finish_block = dim3(256);
    } else if (f.energy) {
        r.finish_fn = step_kernels().energy_reduce;
        r.finish_grid = dim3(1);
        r.finish_block = dim3(1024);
    }
    return hipSuccess;
}

// One kernel node behind `prev` (null: a root of the graph).  p is filled here and must outlive the graph's exec: a launch
// hands it to hipGraphExecKernelNodeSetParams again, with args -- storage the caller owns just as long -- pointing at the new values.
hipError_t add_kernel_node(hipGraph_t graph, hipGraphNode_t prev, hipGraphNode_t *node, hipKernelNodeParams &p, const void *fn, dim3 grid, dim3 block,
                           size_t lds, void **args)
{
    p = hipKernelNodeParams{};
    p.func = const_cast<void *>(fn);
    p.gridDim = grid;
    p.blockDim = block;
    p.sharedMemBytes = unsigned(lds);
    p.kernelParams = args;
    p.extra = nullptr;
    return hipGraphAddKernelNode(node, graph, prev ? &prev : nullptr, prev ? 1 : 0, &p);
}

hipError_t launch_eval_kernels(const EvalArgs &e, hipStream_t stream, hipEvent_t *ev)
{
    LaunchRecipe r;
    hipError_t err = make_recipe(e, r);
    if (err != hipSuccess) return err;
    if (r.tile_fn) {
        void *argv[] = {&r.k};
        err = hipLaunchKernel(r.tile_fn, r.tile_grid, r.tile_block, argv, r.tile_lds, stream);
        if (err != hipSuccess) return err;
    }
    if (ev) {
        err = hipEventRecord(ev[1], stream);
        if (err != hipSuccess) return err;
    }
    if (r.finish_fn) {
        void *argv[] = {&r.f};
        err = hipLaunchKernel(r.finish_fn, r.finish_grid, r.finish_block, argv, 0, stream);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_eval(const EvalArgs &e, hipStream_t stream, hipEvent_t *ev)
{
    if (ev) {
        hipError_t err = hipEventRecord(ev[0], stream);
        if (err != hipSuccess) return err;
    }
    hipError_t rc = launch_eval_kernels(e, stream, ev);
    if (rc == hipSuccess && ev) rc = hipEventRecord(ev[2], stream);
    return rc;
}

// ---- the evaluation as an explicit HIP graph (tile node -> finish node) ----
// The coefficients are kernel ARGUMENTS of both nodes: a launch updates them with hipGraphExecKernelNodeSetParams --
// host-side bookkeeping, nothing on the GPU's timeline -- so a replay follows the reference's coefficient schedule
// (energies/smooth_barrier.py:47-58) without a device-side coefficient buffer and its per-step 8-byte copy (measured
// round 3: 64 x kuhn8 24.3 us per replayed step with that copy against 15.6 us with constant coefficients).
struct EvalGraph {
    LaunchRecipe r;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraphNode_t tile_node = nullptr, finish_node = nullptr;
    hipKernelNodeParams tile_p, finish_p;
    void *tile_argv[1], *finish_argv[1];
    float *own_grad = nullptr;   // the gradient buffer the graph was created with (a launch may name another one)
};

hipError_t eval_graph_create(const EvalArgs &e, EvalGraph **out)
{
    *out = nullptr;
    EvalGraph *g = new EvalGraph();
    hipError_t err = make_recipe(e, g->r);
    g->own_grad = e.grad;
    auto fail = [&](hipError_t code) {
        eval_graph_destroy(g);
        return code;
    };
    if (err != hipSuccess) return fail(err);
    if ((err = hipGraphCreate(&g->graph, 0)) != hipSuccess) return fail(err);
    const LaunchRecipe &r = g->r;
    if (r.tile_fn) {
        g->tile_argv[0] = &g->r.k;
        if ((err = add_kernel_node(g->graph, nullptr, &g->tile_node, g->tile_p, r.tile_fn, r.tile_grid, r.tile_block, r.tile_lds, g->tile_argv)) != hipSuccess)
            return fail(err);
    }
    if (r.finish_fn) {
        g->finish_argv[0] = &g->r.f;
        if ((err = add_kernel_node(g->graph, g->tile_node, &g->finish_node, g->finish_p, r.finish_fn, r.finish_grid, r.finish_block, 0, g->finish_argv)) !=
            hipSuccess)
            return fail(err);
    }
    if ((err = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0)) != hipSuccess) return fail(err);
    *out = g;
    return hipSuccess;
}

hipError_t eval_graph_launch(EvalGraph *g, float c1, float c2, hipStream_t stream, float *energy_copy, float *grad)
{
    hipError_t err;
    const bool coef = g->r.k.c1 != c1 || g->r.k.c2 != c2 || g->r.f.c1 != c1 || g->r.f.c2 != c2;
    // (the gradient's address is an argument of both nodes, the energy copy's of the finish node -- per-launch, like the coefficients)
    if (!grad) grad = g->own_grad;
    if (grad != g->r.f.grad && !g->own_grad) return hipErrorInvalidValue;   // (a graph created without a gradient has no backward kernels)
    const bool moved = grad != g->r.f.grad;
    if (coef || moved) {
        set_coefficients(g->r.k, c1, c2);
        g->r.f.c1 = c1;
        g->r.f.c2 = c2;
        g->r.k.grad = grad;
        if (g->tile_node && (err = hipGraphExecKernelNodeSetParams(g->exec, g->tile_node, &g->tile_p)) != hipSuccess) return err;
    }
    if (coef || moved || g->r.f.energy_copy != energy_copy) {
        if (energy_copy && (!g->finish_node || !g->r.f.energy)) return hipErrorInvalidValue;   // (no node reduces the energy in this graph)
        g->r.f.energy_copy = energy_copy;
        g->r.f.grad = grad;
        if (g->finish_node && (err = hipGraphExecKernelNodeSetParams(g->exec, g->finish_node, &g->finish_p)) != hipSuccess) return err;
    }
    return hipGraphLaunch(g->exec, stream);
}

void eval_graph_destroy(EvalGraph *g)
{
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

// ---- n optimisation steps as one graph (trainer.py:128-133 folded: energy + backward, optimizer.step) ----
// Every step is four kernel nodes in a chain -- tile, finish, adam_moments, adam_apply -- and the steps are chained to each
// other through the parameter (apply of step k writes what tile of step k + 1 reads).  Nothing per step on the host: one launch
// per n steps, the schedule (coefficients, order, bias corrections, step limit) goes in as node arguments beforehand.
struct TrainLoopGraph {
    struct Adam {
        const float *grad;
        float *g1, *g2, *p;
        int64_t n;
        float b1, b2, lr, bias1, bias2, limit;
        unsigned int *ws;
    };
    // One step.  The parameter blocks point at the argument-pointer arrays and those at the recipe and the optimiser's scalars,
    // all inside this struct: the steps are sized once, before the first node is added, and never move.
    struct Step {
        LaunchRecipe r;
        Adam a;
        hipGraphNode_t tile = nullptr, finish = nullptr, moments = nullptr, apply = nullptr;
        hipKernelNodeParams tile_p, finish_p, moments_p, apply_p;
        void *tile_argv[1], *finish_argv[1], *moments_argv[7], *apply_argv[8];
    };
    std::vector<Step> steps;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

hipError_t train_loop_create(const EvalArgs &e, float *param, float *g1, float *g2, int64_t n_param, void *ws, int n_iters, TrainLoopGraph **out)
{
    *out = nullptr;
    if (n_iters < 1 || n_iters > 4096 || n_param < 1 || !e.grad || !e.energy) return hipErrorInvalidValue;
    TrainLoopGraph *g = new TrainLoopGraph();
    auto fail = [&](hipError_t code) {
        train_loop_destroy(g);
        return code;
    };
    g->steps.resize(size_t(n_iters));
    const StepKernels sk = step_kernels();
    const dim3 adam_blocks(adam_grid(n_param));
    hipError_t err;
    if ((err = hipGraphCreate(&g->graph, 0)) != hipSuccess) return fail(err);
    // the optimiser's two-dword scratch of every step, zeroed once per launch
    hipGraphNode_t prev = nullptr;
    {
        hipMemsetParams m = {};
        m.dst = ws;
        m.elementSize = 4;
        m.width = size_t(2 * n_iters);
        m.height = 1;
        m.value = 0;
        if ((err = hipGraphAddMemsetNode(&prev, g->graph, nullptr, 0, &m)) != hipSuccess) return fail(err);
    }
    for (int k = 0; k < n_iters; ++k) {
        TrainLoopGraph::Step &s = g->steps[size_t(k)];
        EvalArgs ek = e;
        ek.x = param;
        ek.energy = e.energy + k;
        if ((err = make_recipe(ek, s.r)) != hipSuccess) return fail(err);
        const LaunchRecipe &r = s.r;
        // a chain: every node behind the one added before it
        auto add = [&](hipGraphNode_t *node, hipKernelNodeParams &p, const void *fn, dim3 grid, dim3 block, size_t lds, void **args) {
            const hipError_t rc = add_kernel_node(g->graph, prev, node, p, fn, grid, block, lds, args);
            if (rc == hipSuccess) prev = *node;
            return rc;
        };
        if (r.tile_fn) {
            s.tile_argv[0] = &s.r.k;
            if ((err = add(&s.tile, s.tile_p, r.tile_fn, r.tile_grid, r.tile_block, r.tile_lds, s.tile_argv)) != hipSuccess) return fail(err);
        }
        if (r.finish_fn) {
            s.finish_argv[0] = &s.r.f;
            if ((err = add(&s.finish, s.finish_p, r.finish_fn, r.finish_grid, r.finish_block, 0, s.finish_argv)) != hipSuccess) return fail(err);
        }
        TrainLoopGraph::Adam &a = s.a;
        a = TrainLoopGraph::Adam{e.grad, g1, g2, param, n_param, 0.9f, 0.999f, 0.f, 1.f, 1.f, -1.f, static_cast<unsigned int *>(ws) + 2 * k};
        void **am = s.moments_argv, **aa = s.apply_argv;
        am[0] = &a.grad, am[1] = &a.g1, am[2] = &a.g2, am[3] = &a.n, am[4] = &a.b1, am[5] = &a.b2, am[6] = &a.ws;
        aa[0] = &a.p, aa[1] = &a.g1, aa[2] = &a.n, aa[3] = &a.lr, aa[4] = &a.bias1, aa[5] = &a.bias2, aa[6] = &a.limit, aa[7] = &a.ws;
        if ((err = add(&s.moments, s.moments_p, sk.adam_moments, adam_blocks, dim3(256), 0, am)) != hipSuccess) return fail(err);
        if ((err = add(&s.apply, s.apply_p, sk.adam_apply, adam_blocks, dim3(256), 0, aa)) != hipSuccess) return fail(err);
    }
    if ((err = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0)) != hipSuccess) return fail(err);
    *out = g;
    return hipSuccess;
}

hipError_t train_loop_launch(TrainLoopGraph *g, const TrainLoopStep *steps, float lr, float b1, float b2, hipStream_t stream)
{
    hipError_t err;
    for (size_t k = 0; k < g->steps.size(); ++k) {
        TrainLoopGraph::Step &st = g->steps[k];
        LaunchRecipe &r = st.r;
        const TrainLoopStep &s = steps[k];
        if (r.k.c1 != s.c1 || r.k.c2 != s.c2 || r.k.order != s.order || r.f.c1 != s.c1 || r.f.c2 != s.c2) {
            set_coefficients(r.k, s.c1, s.c2);
            r.f.c1 = s.c1;
            r.f.c2 = s.c2;
            r.k.order = s.order;
            if (st.tile && (err = hipGraphExecKernelNodeSetParams(g->exec, st.tile, &st.tile_p)) != hipSuccess) return err;
            if (st.finish && (err = hipGraphExecKernelNodeSetParams(g->exec, st.finish, &st.finish_p)) != hipSuccess) return err;
        }
        TrainLoopGraph::Adam &a = st.a;
        if (a.b1 != b1 || a.b2 != b2) {
            a.b1 = b1;
            a.b2 = b2;
            if ((err = hipGraphExecKernelNodeSetParams(g->exec, st.moments, &st.moments_p)) != hipSuccess) return err;
        }
        if (a.lr != lr || a.bias1 != s.bias1 || a.bias2 != s.bias2 || a.limit != s.limit) {
            a.lr = lr;
            a.bias1 = s.bias1;
            a.bias2 = s.bias2;
            a.limit = s.limit;
            if ((err = hipGraphExecKernelNodeSetParams(g->exec, st.apply, &st.apply_p)) != hipSuccess) return err;
        }
    }
    return hipGraphLaunch(g->exec, stream);
}

void train_loop_destroy(TrainLoopGraph *g)
{
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

}  // namespace tsamd
