/*
 * tssplat_amd -- C ABI of the MI355X (gfx950) tet-sphere geometry-energy path.
 *
 * This is the drop-in boundary for the one hot path of gmh14/tssplat: the
 * per-iteration energy  E = c1 * 1/2 |L G x|^2 + c2 * sum_e max(-det F_e, 0)^p
 * and its analytic gradient.  Every entry point below replaces one piece of the
 * reference's native extension `tet_spheres.tet_spheres_ext`
 * (citations into /root/reference/tssplat_ext/tet_spheres/):
 *
 *   tsamd_create            <- TetSpheres::TetSpheres(int nv, double*, int ntet, int*)   tet_spheres.cpp:119-126
 *                              + TetSpheres::init                                        tet_spheres.cpp:140-203
 *                              + the pybind array constructor                            tet_spheres.cpp:234-258
 *   tsamd_create_with_operator <- the same, with the element Laplacian that the reference takes from libpgo
 *                              (pgo_create_tet_biharmonic_gradient_matrix, tet_spheres.cpp:148) passed as data
 *   tsamd_create_from_veg   <- TetSpheres::TetSpheres(const std::string& filename)       tet_spheres.cpp:108-117
 *   tsamd_destroy           <- TetSpheres::~TetSpheres                                   tet_spheres.cpp:128-138
 *   tsamd_forward           <- tet_spheres_smooth_barrier          (forward)             tet_spheres_cuda.cu:118-195
 *   tsamd_backward          <- tet_spheres_smooth_barrier_backward (backward)            tet_spheres_cuda.cu:197-263
 *   tsamd_forward_backward  <- both of the above fused into one pass (no reference twin:
 *                              the reference recomputes G x in backward, .cu:221)
 *   tsamd_scale             <- the cublasSscal by gradH.item() at                        tet_spheres_cuda.cu:257-258
 *   tsamd_grad_limit        <- tet_spheres_grad_limit (intended semantics, see below)    tet_spheres_cuda.cu:265-303
 *   tsamd_num_vertices/_tets<- TetSpheres::n / ::nele                                    tet_spheres.h:40
 *   tsamd_last_error        <- the stderr line + std::runtime_error of cudaUtils.h:10-44
 *
 * Plain pointers and sizes only; no torch, no C++ types.  All `*_dev` pointers
 * are HIP device pointers on the device the handle was created on; `stream`
 * is a hipStream_t passed as void* (NULL = the null stream).  No entry point
 * synchronises the host with the device except tsamd_create / tsamd_destroy /
 * tsamd_read_energy_terms.  Every function returns 0 on success and a nonzero
 * tsamd_status otherwise; the message is available from tsamd_last_error()
 * (thread-local).  A handle is not re-entrant and is single-stream: its staging rows, per-tile partials and
 * energy terms are per-handle scratch, so evaluations of ONE handle must be ordered (one stream, or events between
 * streams); different handles are independent (same rule as the reference's per-object scratch,
 * tet_spheres.h:36-40).
 */
#ifndef TSSPLAT_AMD_H
#define TSSPLAT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsamd_handle tsamd_handle;

typedef enum tsamd_status {
    TSAMD_OK = 0,
    TSAMD_ERR_INVALID_ARGUMENT = 1,  /* null pointer, negative size, index out of range           */
    TSAMD_ERR_BAD_MESH = 2,          /* non-manifold face (>2 tets), singular rest tet             */
    TSAMD_ERR_NO_DEVICE = 3,         /* no HIP device / not a gfx950-class device                  */
    TSAMD_ERR_HIP = 4,               /* a HIP runtime call failed (text in tsamd_last_error)       */
    TSAMD_ERR_IO = 5,                /* tsamd_create_from_veg: unreadable or malformed file        */
    TSAMD_ERR_TILING = 6,            /* mesh cannot be tiled into the LDS budget                   */
    TSAMD_ERR_HOST_ONLY = 7          /* device entry point called on a host_only handle            */
} tsamd_status;

/* Zero-initialise, set struct_size = sizeof(tsamd_options) and abi_version = TSAMD_ABI_VERSION, override what you need. */
typedef struct tsamd_options {
    int32_t struct_size;
    int32_t device;            /* HIP device ordinal; -1 = current device                          */
    int32_t lds_budget_bytes;  /* LDS per workgroup a tile may use; 0 = 81920 (two workgroups per gfx950 CU) */
    int32_t max_threads;       /* workgroup size cap, multiple of 64, <= 768 (see slots_per_thread for the other lane layouts); 0 = 768 */
    int32_t target_owned;      /* owned tets per tile the partitioner aims for; 0 = auto: the fullest tiles that fit, except that a
                                * plan of <= 1024 tiles built with lds_budget_bytes = max_threads = target_owned = 0 is re-tiled at
                                * 768 (a small batch pays for a tile's latency, not for its halo) */
    int32_t lane_search_sweeps;/* sweeps of the search that seats a tile's tets on the lanes against LDS bank conflicts of the neighbour
                                * gathers (plan time, ~1.5 ms per tile, sweep and host thread; tile kernel -2 %): 0 = 2, -1 = none
                                * (tets stay in Morton order).  Results do not depend on it beyond the order of fp32 sums. */
    int32_t host_only;         /* 1 = build the tiling plan only, never touch HIP (CPU tests)       */
    int32_t num_threads;       /* host threads used to build the plan; 0 = hardware concurrency     */
    int32_t debug_flags;       /* bit1 = no LDS-conflict-aware ordering at all (measurements); bit2 = no shared index planes: every
                                * tile is its own index representative (tsamd_get_index_reps; same results, bit for bit); bit3 = no regular-batch addressing: every tile
                                * and finish vertex reads its own ids, destinations and lists (tsamd_get_regular_batch reports period 0;
                                * same results, bit for bit); other bits ignored */
    int32_t slots_per_thread;  /* tets per lane: 0 = 2.  Lane layouts with a kernel: 2 (max_threads <= 768, two 80 KiB workgroups per
                                * CU: the default, every operator variant); 3 (max_threads <= 512, or <= 1024 for one workgroup per
                                * CU) and 4 (max_threads <= 768): fewer, fatter waves, built-in operator only -- with lds_budget_bytes
                                * up to 163840 these hold a whole ~3 k-tet sphere as ONE tile (no halo, no shared vertices).
                                * Anything else is TSAMD_ERR_INVALID_ARGUMENT. */
    int32_t rebuild_dminv;     /* 0 = auto: stream Dm^-1, except for plans of 513 ... 2 048 tiles built with default tiling options
                                * whose tiles the rebuilt form does not shrink (a few rounds of workgroups of small spheres: 256 x 3 k-tet
                                * spheres 24.8 -> 22.8 us per step), which rebuild it;
                                * 2 = always stream; 1 = always rebuild:
                                * keep rest positions (16 B per tile vertex) instead of the Dm^-1 planes (36 of the
                                * 52 B per tile slot) and invert Dm per slot in fp32 registers: 45 % fewer bytes per
                                * evaluation, entries of Dm^-1 within 2.8e-7 relative of the exact inverse instead of
                                * 5.9e-8 (double -> fp32 rounding, tet_spheres.cpp:43-45).  Not with an explicit operator. */
    int32_t abi_version;       /* must be TSAMD_ABI_VERSION of the header the caller was compiled against: ABI 1 and 2 shared one
                                * struct size while two fields changed their meaning in place, so a stale caller was re-interpreted
                                * instead of rejected.  From ABI 3 on the size changes with the version AND the version is checked. */
} tsamd_options;

/* Introspection of the tiling plan (host side; valid for host_only handles too). */
typedef struct tsamd_plan_info {
    int64_t n_vertices, n_tets;
    int64_t n_tiles;
    int64_t n_components;        /* face-connected components (= tet-spheres)                       */
    int64_t total_slots;         /* sum over tiles of owned + halo tets                             */
    int64_t total_tile_vertices; /* sum over tiles of local vertices                                */
    int64_t shared_vertex_copies;/* tile-vertex copies that go through the staging buffer           */
    int64_t finish_vertices;     /* global vertices written by the finish kernel                    */
    int64_t device_bytes;        /* bytes of plan data resident in HBM                              */
    int32_t max_slots, max_tile_vertices, block_threads, lds_bytes;
    int32_t slots_per_thread;
    int32_t n_planes;            /* dword planes per tile slot: 13; 22 with an explicit element operator (18 when it is symmetric); 4 with rebuild_dminv */
} tsamd_plan_info;

/* How the plan was cut, next to what a halo-free plan would carry (host side; valid for host_only handles too).  Every
 * owned tet is a slot that has to be there; the halo slots and the staged rows exist only because tet-spheres are cut into
 * several tiles, so owned_tets is the lower bound of the slots and 0 that of the rows, and min_tiles = the fewest tiles
 * that could hold total_slots at all. */
typedef struct tsamd_partition_info {
    int64_t owned_tets;          /* = n_tets                                                         */
    int64_t halo_slots;          /* total_slots - owned_tets                                         */
    int64_t staged_rows;         /* = shared_vertex_copies                                           */
    int64_t n_tiles;
    int64_t tile_capacity;       /* slots one tile can hold: lanes x slots per lane of the plan's launch shape          */
    int64_t min_tiles;           /* ceil(total_slots / tile_capacity)                                */
    int64_t cut_components;      /* tet-spheres too large for one tile                               */
    int64_t bisection_components;/* ... of which kept the coordinate bisection's tiles (the compact cells did not beat them) */
    int64_t cut_templates;       /* ... of which were cut themselves: the others are copies of one of them and took its cut over */
    double mean_fill, max_fill;  /* slots of a tile over tile_capacity                               */
} tsamd_partition_info;

/* One tile of the plan, as host pointers into the handle (valid until tsamd_destroy).
 * Exists so tests can replay the exact data the kernels consume. */
typedef struct tsamd_tile_view {
    int32_t n_slots, n_owned, s_pad, n_verts, n_excl;
    int64_t stage_off;
    int32_t n_rows;            /* rows of the tile's per-vertex force array = most slots any tile vertex meets (<= 64) */
    int32_t rec_base;          /* LDS byte address of record 0: the neighbour tokens are (rec_base + 48 idx) / 4 + rot    */
    const uint32_t *planes;    /* n_planes planes of s_pad dwords: lv01, lv23, nb01, nb23, dminv[0..8]
                                * (+ L[e,e], L[e,n_0..3], L[n_0..3,e] as fp32 with an explicit operator);
                                * a 16-bit vertex field = local vertex | rank << 10                                      */
    const uint16_t *row_start; /* 72 entries: row r of the force array starts at entry row_start[r]; entry (v, r) of
                                * local vertex v = row_start[r] + v (vertices are numbered by falling slot count)        */
    const int32_t *gvid;       /* n_verts global vertex ids (a vertex met by more than 64 slots appears several times)   */
    const int32_t *vdst;       /* n_verts destinations: >= 0 row of grad (the vertex is this tile's alone), < 0: staging
                                * row ~vdst, summed by the finish kernel                                                  */
    const int32_t *slot_tet;   /* s_pad global tet ids (-1 = padding)                                                     */
    const float *rest;         /* rebuild_dminv plans: n_verts x float4 rest positions (tile vertex order), else NULL    */
} tsamd_tile_view;

const char *tsamd_last_error(void);
const char *tsamd_version(void);
/* Bumped whenever a struct layout or a signature of this header changes incompatibly (0.1 had no such call: a caller that
 * cannot find the symbol is talking to an older library).  Compare with TSAMD_ABI_VERSION of the header you compiled against. */
#define TSAMD_ABI_VERSION 3
int32_t tsamd_abi_version(void);

/*
 * rest_xyz: n_vertices*3 float32 (host), tets: n_tets*4 int32 (host, 0-based).
 * Exactly the arrays energies/smooth_barrier.py:38-40 hands to TetSpheres(v_flat, f_flat).
 * The rest shape is frozen here (positions promoted to double, Dm^-1 built in
 * double and rounded to fp32 -- tet_spheres.cpp:252-255, :43-45).
 */
int tsamd_create(const float *rest_xyz, int64_t n_vertices, const int32_t *tets, int64_t n_tets,
                 const tsamd_options *options, tsamd_handle **out);
int tsamd_create_from_veg(const char *path, const tsamd_options *options, tsamd_handle **out);
/*
 * Same as tsamd_create, with the element operator L of the smoothness term H = (L (x) I9) G x given as data
 * (SURVEY 8(b) "optional create inputs: explicit CSR adjacency + weights").  The reference takes L from
 * libpgo -- pgo_create_tet_biharmonic_gradient_matrix(geo, faceNeighbor=1, scale=0), tet_spheres.cpp:148 --
 * whose source is not part of the reference; tsamd_create ASSUMES the uniform face-adjacency umbrella
 * (L[e,e] = number of face neighbours, L[e,e'] = -1).  This entry point substitutes any other operator with
 * the same sparsity (e.g. the matrix libpgo really builds, dumped by tools/pin_L_with_pypgo.py, or the
 * row-scaled scale=1 variant): m x m CSR over tets, double values (rounded to fp32 like the reference's
 * matrix values, tet_spheres.cpp:43-45), 0-based.  Entries must lie on the diagonal or on a face adjacency of
 * the mesh (duplicates are summed); anything else is TSAMD_ERR_INVALID_ARGUMENT.  L need not be symmetric:
 * the gradient applies L^T explicitly.  Cost: 9 more fp32 planes per tile slot (88 instead of 52 bytes); 5 (72 bytes) when
 * the operator is symmetric after the rounding to fp32 -- its weights are then stored once and serve both passes.
 */
int tsamd_create_with_operator(const float *rest_xyz, int64_t n_vertices, const int32_t *tets, int64_t n_tets,
                               const int64_t *op_rowptr, const int32_t *op_col, const double *op_val,
                               const tsamd_options *options, tsamd_handle **out);
void tsamd_destroy(tsamd_handle *h);

int64_t tsamd_num_vertices(const tsamd_handle *h);
int64_t tsamd_num_tets(const tsamd_handle *h);
int tsamd_get_plan_info(const tsamd_handle *h, tsamd_plan_info *out);
int tsamd_get_partition_info(const tsamd_handle *h, tsamd_partition_info *out);
int tsamd_get_tile(const tsamd_handle *h, int64_t tile, tsamd_tile_view *out);
/* finish lists: vertex k (global id vid[k]) = sum of staging rows [off[k], off[k+1]);
 * idx[tile.stage_off + j] = the staging row the tile's j-th shared tile vertex (in tile vertex order) writes -- the same
 * rows tsamd_tile_view.vdst names (off[n_finish] entries) */
int tsamd_get_finish_lists(const tsamd_handle *h, int64_t *n_finish, const int32_t **vid,
                           const int32_t **off, const int32_t **idx);
/* rep[t], one entry per tile = the tile whose index planes (planes 0-3) and row table the kernels read for tile t: the first tile
 * of the plan that carries the same bytes (the same tile of an earlier copy of one template), t itself if there is none.  Tile t's
 * own bytes (tsamd_get_tile) are byte-equal to its representative's. */
int tsamd_get_index_reps(const tsamd_handle *h, const int32_t **rep);
/* Regular batch: out7 = {period, copies, V, S, K, div_mul, div_shift}.  period > 0: the plan is `copies` >= 2 repetitions of its
 * first `period` tiles -- tile t is copy c = t / period of template tile r = t % period, and with V vertices, S staging rows and K
 * finish vertices per copy
 *   gvid[t][v] = gvid[r][v] + c V;   vdst[t][v] = vdst[r][v] + c V where that is >= 0, ~vdst[t][v] = ~vdst[r][v] + c S where it is < 0;
 *   vid[k] = vid[k % K] + (k / K) V;   off[k] = off[k % K] + (k / K) S   (k = n_finish included),
 * every entry compared at create time.  The kernels then read the template's entries (bytes every copy shares) and add the copy's
 * constants; c = (t * div_mul) >> div_shift in 64 bits, exact for every tile of the plan.  period = 0 (and zeros throughout): anything
 * else -- a single copy, mixed templates, one odd sphere -- or debug_flags bit3; the kernels read every tile's own entries.  Same
 * results either way, bit for bit. */
int tsamd_get_regular_batch(const tsamd_handle *h, int64_t *out7);
/* face adjacency computed at create time: 4 ints per tet, -1 = boundary face */
int tsamd_get_adjacency(const tsamd_handle *h, const int32_t **nbr);

/*
 * energy_dev: 1 float, receives E = c1*E_s + c2*E_b.  x_dev: n_vertices*3 floats.
 * order: 2 or 4 are meaningful; any other value makes the penalty term 0
 * (tet_spheres_cuda.cu:57-63).
 */
int tsamd_forward(tsamd_handle *h, const float *x_dev, float c1, float c2, int order,
                  void *stream, float *energy_dev);
/*
 * grad_dev: n_vertices*3 floats, overwritten with grad_out * dE/dx.
 * grad_out_dev: 1 float on the device (the autograd grad_output), or NULL for 1.0.
 * Read on the device: no .item() style host sync (contrast tet_spheres_cuda.cu:257).
 */
int tsamd_backward(tsamd_handle *h, const float *x_dev, const float *grad_out_dev, float c1, float c2,
                   int order, void *stream, float *grad_dev);
/* One pass producing both; energy_dev may be NULL. */
int tsamd_forward_backward(tsamd_handle *h, const float *x_dev, const float *grad_out_dev, float c1,
                           float c2, int order, void *stream, float *energy_dev, float *grad_dev);
/*
 * The same evaluation with the two coefficients read ON THE DEVICE: coef_dev = {c1, c2} (2 floats).  The
 * reference's schedule changes c1 and c2 every iteration (energies/smooth_barrier.py:47-58); with the
 * coefficients in device memory a HIP graph captured once replays across iterations (the caller updates
 * coef_dev, e.g. with a captured copy from pinned host memory).  energy_dev or grad_dev may be NULL (not both).
 * No reference twin: the reference launches ~10 library calls per evaluation from the host every time.
 */
int tsamd_evaluate_dev_coef(tsamd_handle *h, const float *x_dev, const float *grad_out_dev, const float *coef_dev,
                            int order, void *stream, float *energy_dev, float *grad_dev);
/*
 * The fused evaluation as an instantiated HIP graph (tile kernel -> finish kernel), for batches whose 10-30 us of kernels
 * drown in per-step host work (the reference pays ~80 us of launches, descriptor set-up and three blocking device reads
 * per iteration at trainer.py:94,130).  tsamd_graph_create bakes in the pointers (x_dev, grad_out_dev -- may be NULL --,
 * energy_dev, grad_dev; at least one of the two outputs) and `order`; tsamd_graph_launch replays it on `stream` with the
 * coefficients of THIS iteration -- they are kernel arguments of the graph's nodes and are updated on the host
 * (hipGraphExecKernelNodeSetParams), so following the reference's schedule (energies/smooth_barrier.py:47-58) costs
 * nothing on the device.  Same kernels, same results as tsamd_forward_backward.  The graph borrows the handle's scratch:
 * the single-stream rule of the handle applies, and the handle must outlive the graph.
 */
typedef struct tsamd_graph tsamd_graph;
int tsamd_graph_create(tsamd_handle *h, const float *x_dev, const float *grad_out_dev, int order, float *energy_dev,
                       float *grad_dev, tsamd_graph **out);
int tsamd_graph_launch(tsamd_graph *graph, float c1, float c2, void *stream);
/* The same replay with its outputs redirected for THIS launch (per-launch arguments of the graph's nodes, like the coefficients):
 *   energy_copy_dev  the energy is ALSO written there (one float; NULL = not): how an energy exchange across GPUs gets a launch's
 *                    value into its own ring slot without a copy on the stream (tssplat_amd/sharding.py: OverlappedEnergyAllReduce);
 *                    requires a graph created with energy_dev;
 *   grad_dev         the gradient goes THERE instead of the buffer the graph was created with ([n_vertices, 3] floats; NULL = the
 *                    graph's own): a caller that hands every evaluation's gradient on (x.grad of a training loop) gets it in a
 *                    fresh buffer without a device copy; requires a graph created with grad_dev. */
int tsamd_graph_launch_to(tsamd_graph *graph, float c1, float c2, void *stream, float *energy_copy_dev, float *grad_dev);
void tsamd_graph_destroy(tsamd_graph *graph);

/* n_iters optimisation steps as ONE HIP graph: per step the evaluation above (energy into energy_ring_dev[k], gradient into
 * grad_dev, upstream gradient 1) followed by tsamd_adam_uniform_step on param_dev with that gradient -- the sequence
 * loss.backward(); optimizer.step() of /root/reference/trainer.py:130-133 for a loss that is the energy alone, with nothing on
 * the host between the steps.  The pointers are baked in (param_dev [n_vertices, 3] is read and updated in place; g1_dev /
 * g2_dev are the optimiser's moments; workspace_dev: tsamd_train_loop_workspace_bytes(n_iters)).  A launch takes the schedule of
 * its n_iters steps -- c1[k], c2[k], order[k] (energies/smooth_barrier.py:47-63), the optimiser's step number of the first one
 * (first_step >= 1: bias corrections 1 - beta^step as in tsamd_adam_uniform_step) and optionally grad_limit[k] (NULL or < 0:
 * none) -- as kernel-node arguments.  Same single-stream rule as the handle; the handle must outlive the loop. */
typedef struct tsamd_train_loop tsamd_train_loop;
int64_t tsamd_train_loop_workspace_bytes(int32_t n_iters);
int tsamd_train_loop_create(tsamd_handle *h, float *param_dev, float *grad_dev, float *g1_dev, float *g2_dev, float *energy_ring_dev,
                            void *workspace_dev, int32_t n_iters, tsamd_train_loop **out);
int tsamd_train_loop_launch(tsamd_train_loop *loop, const float *c1, const float *c2, const int32_t *order, float lr, float beta1, float beta2,
                            int64_t first_step, const float *grad_limit, void *stream);
void tsamd_train_loop_destroy(tsamd_train_loop *loop);

/* Blocking read of the last evaluation's (E_s, E_b) in double, for diagnostics. */
int tsamd_read_energy_terms(tsamd_handle *h, void *stream, double *terms_host2);

/*
 * Kernel timing for bench.py's roofline leg.  While enabled, every evaluation records HIP
 * events on its stream around the tile kernel and the finish kernel (no host sync).
 * tsamd_get_timing synchronises those events, returns the accumulated milliseconds and the
 * number of evaluations, and clears the record.
 */
int tsamd_set_timing(tsamd_handle *h, int enable);
int tsamd_get_timing(tsamd_handle *h, double *tile_kernel_ms, double *finish_kernel_ms, int64_t *evaluations);

/* out[i] = in[i] * (*scalar_dev); in == out allowed. */
int tsamd_scale(const float *in_dev, const float *scalar_dev, float *out_dev, int64_t n, void *stream);
/*
 * In-place step clamp with the semantics the reference intended
 * (utils/optimizer.py:84-86: if max|g| > threshold: g *= s / max|g|), not the
 * shipped bug that reads g[0] (tet_spheres_cuda.cu:278).  No host sync.
 * workspace_dev: >= tsamd_grad_limit_workspace_bytes() bytes of scratch.
 */
int64_t tsamd_grad_limit_workspace_bytes(void);
int tsamd_grad_limit(float *grad_dev, int64_t n, float s_threshold, float s, void *workspace_dev,
                     void *stream);

/*
 * SURVEY 8(f) row 3 -- the optimiser step that follows every backward: one fused AdamUniform step
 * (reference utils/optimizer.py:38-89) over a contiguous float32 parameter, in place, no host sync
 * (the reference takes two .max() reductions and, with grad_limit, a Python `if s > m` per step).
 *   g1 = b1 g1 + (1-b1) grad;  g2 = b2 g2 + (1-b2) grad^2;            optimizer.py:61-62
 *   gr = (g1 / (1-b1^step)) / (1e-8 + max sqrt(g2 / (1-b2^step)));    optimizer.py:67-74
 *   if grad_limit > 0 and max|gr| > grad_limit: gr *= grad_limit / max|gr|;   optimizer.py:84-86
 *   param -= lr * gr                                                   optimizer.py:88
 * `step` is the 1-based count AFTER the increment of optimizer.py:55.  workspace_dev: >= 16 bytes.
 * Non-finite gradients: a +inf entry makes both maxima inf, so every finite entry of param stays as it is, bit for bit,
 * and the entry itself becomes NaN (g1, g2 inf there) -- what the reference's torch chain gives too.
 * A NaN entry DEPARTS from the reference: the maxima here drop NaN (fmaxf), so every other entry is stepped as if that entry
 * were absent and only its own param, g1 and g2 become NaN, where torch's .max() propagates NaN into every entry.
 */
int tsamd_adam_uniform_step(float *param_dev, const float *grad_dev, float *g1_dev, float *g2_dev, int64_t n,
                            float lr, float beta1, float beta2, int64_t step, float grad_limit,
                            void *workspace_dev, void *stream);

/*
 * SURVEY 8(f) row 2 -- the surface glue around the energy in every iteration
 * (reference geometry/tetmesh_geometry.py:27-66) and the one-off boundary extraction
 * (geometry/mesh_utils.py:5-35).  All kernels are per-vertex gathers over fixed lists: no atomics,
 * bitwise repeatable.  float32 values, int32 indices, [k,3] arrays row-major and contiguous.
 */
typedef struct tsamd_surface tsamd_surface;

/* get_surface_vf(elem) (mesh_utils.py:5-35), host only: boundary triangles (faces of exactly one tet) ordered
 * by their sorted vertex triple, oriented like the tet-local pattern they come from, vertex ids compacted to
 * their rank in `surface_vid` (ascending tet-vertex ids).  Call once with surface_vid = faces = NULL to get the
 * sizes, then with buffers of *n_surface_vertices and 3 * *n_faces entries (capacities passed in the counters). */
int tsamd_extract_surface(const int32_t *tets, int64_t n_tets, int64_t n_vertices, int32_t *surface_vid,
                          int64_t *n_surface_vertices, int32_t *faces, int64_t *n_faces);

/* Device copy of the surface topology: surface_vid[ns] (TetMeshGeometry.surface_vid, tetmesh_geometry.py:146),
 * faces[nf,3] indexing surface vertices (surface_fid, :148).  Host pointers; device < 0 = current device. */
int tsamd_surface_create(const int32_t *surface_vid, int64_t n_surface_vertices, const int32_t *faces, int64_t n_faces,
                         int64_t n_tet_vertices, int device, tsamd_surface **out);
void tsamd_surface_destroy(tsamd_surface *s);

/* v_pos = tet_v[surface_vid]  (tetmesh_geometry.py:33) and its adjoint: grad_tet_v[n_tet_vertices,3] is
 * overwritten (zero, then the rows of grad_v_pos scattered; accumulated if surface_vid has duplicates). */
int tsamd_surface_positions(const tsamd_surface *s, const float *tet_v_dev, void *stream, float *v_pos_dev);
int tsamd_surface_positions_backward(const tsamd_surface *s, const float *grad_v_pos_dev, void *stream,
                                     float *grad_tet_v_dev);

/* _compute_vertex_normal() (tetmesh_geometry.py:39-66): face normals (v1-v0)x(v2-v0) summed per vertex,
 * |n|^2 <= 1e-20 -> (0,0,1), n / max(|n|, 1e-12).  raw_dev (optional, [ns,3]) receives the unnormalised sums,
 * which the backward needs.  Backward: grad_v_pos = (d v_nrm / d v_pos)^T grad_nrm; workspace: 12 * ns bytes. */
int tsamd_vertex_normals(const tsamd_surface *s, const float *v_pos_dev, void *stream, float *v_nrm_dev, float *raw_dev);
int tsamd_vertex_normals_backward(const tsamd_surface *s, const float *v_pos_dev, const float *raw_dev,
                                  const float *grad_nrm_dev, void *workspace_dev, void *stream, float *grad_v_pos_dev);

/* ------------------------------------------------------------------------------------------------------------------
 * Renderer slice: the nvdiffrast operators the reference's renderer calls,
 *   tsamd_rasterize            <- dr.rasterize(ctx, pos_clip, tri, resolution=[H, W], grad_db=False)[0]   renderers/mesh_rasterizer.py:103
 *   tsamd_interpolate          <- dr.interpolate(attr, rast, tri)[0]                                     renderers/mesh_rasterizer.py:117,145,153
 *   tsamd_interpolate_backward <- the backward of the latter w.r.t. attr and rast's (u, v)
 *   tsamd_rasterize_backward, tsamd_antialias* (below) <- the backward of dr.rasterize, dr.antialias and its backward   :103,107,128
 * nvdiffrast is a separate library (not vendored by the reference, version unpinned): the semantics implemented are a
 * restatement of its published algorithm, fixed in every detail by oracle/raster_oracle.py -- clip-space input, OpenGL
 * conventions (row 0 = bottom), no culling, nearest depth, output (u, v, z/w, triangle_id + 1), 0 = background.  PARITY
 * UNPINNED (no nvdiffrast here).  Clipping: against the near plane (z + w >= 0) for triangles with a vertex at w <= 0 (the
 * clipped polygon is rasterised under the triangle's own id; pixels beyond the far plane or the image fail their own tests).
 * Not offered: depth peeling, `ranges`, image-space derivatives (grad_db).  Limits: height, width <= 8192 (window coordinates
 * are snapped to 1/256 pixel and kept within +-16384 pixels; a triangle with a vertex beyond that guard band, or a non-finite
 * one, is dropped whole), n_triangles <= 2^24 - 1 (the id + 1 travels as a float32).  Stateless: the caller owns all buffers and
 * the current HIP device is used.  pos_clip_dev: [batch, n_vertices, 4] f32; tri_dev: [n_triangles, 3] i32;
 * rast: [batch, height, width, 4] f32; attr_dev: [attr_batch (1 or batch), n_vertices, n_channels] f32.
 */
/* workspace: one 64-bit depth key per pixel, one 16-byte snapped vertex per (view, vertex), one flag per view */
int64_t tsamd_rasterize_workspace_bytes(int64_t batch, int64_t n_vertices, int32_t height, int32_t width);
/* pair_masks_out_dev (OPTIONAL, tsamd_pair_masks_bytes(batch, height, width) bytes): a by-product for tsamd_antialias_prepare --
 * per 64 consecutive pixels two 64-bit words, bit l = pixel 64 k + l and its right (word 0) / upper (word 1) neighbour show
 * two different triangles.  The resolve pass has the ids in hand; without it the antialias side reads `rast` back to find them. */
int64_t tsamd_pair_masks_bytes(int64_t batch, int32_t height, int32_t width);
int tsamd_rasterize(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                    int32_t height, int32_t width, void *workspace_dev, float *rast_out_dev, void *pair_masks_out_dev, void *stream);
/* A pixel whose id names no triangle of tri_dev (id > n_triangles, e.g. a rast image made with another list) or a triangle
 * with a vertex index outside [0, n_vertices) is treated as background: zero output, zero gradient, nothing read or written
 * out of bounds. */
int tsamd_interpolate(const float *attr_dev, int64_t attr_batch, int64_t n_vertices, int32_t n_channels, const float *rast_dev,
                      const int32_t *tri_dev, int64_t n_triangles, int64_t batch, int32_t height, int32_t width, float *out_dev, void *stream);
/* grad_attr_dev ([attr_batch, n_vertices, n_channels]) is zero-filled and accumulated by the call; grad_rast_dev
 * ([batch, height, width, 4], channels 2-3 = 0) may be NULL. */
int tsamd_interpolate_backward(const float *attr_dev, int64_t attr_batch, int64_t n_vertices, int32_t n_channels, const float *rast_dev,
                               const int32_t *tri_dev, int64_t n_triangles, int64_t batch, int32_t height, int32_t width, const float *grad_out_dev,
                               float *grad_attr_dev, float *grad_rast_dev, void *stream);

/* Gradient of tsamd_rasterize w.r.t. pos_clip from the gradient of its (u, v) outputs (what flows back from
 * tsamd_interpolate_backward's grad_rast; z/w and the id carry none).  grad_pos_dev [batch, n_vertices, 4] is zero-filled and
 * accumulated by the call.  <- the backward of dr.rasterize(..., grad_db=False), renderers/mesh_rasterizer.py:103 */
int tsamd_rasterize_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                             int32_t height, int32_t width, const float *rast_dev, const float *grad_rast_dev, float *grad_pos_dev, void *stream);

/* tsamd_antialias <- dr.antialias(color, rast, pos_clip, tri, topology_hash=None, pos_gradient_boost=1.0)   renderers/mesh_rasterizer.py:107,128
 * -- the only differentiable path from the alpha image to the geometry.  Every pair of adjacent pixels with different
 * triangle ids is analysed: the closer triangle's silhouette edge that passes between the two pixel centres blends the two
 * colours by the position of the crossing (specification: oracle/raster_oracle.py; PARITY UNPINNED like the rest of the slice).
 * edge_partner_dev [3 * n_triangles] i32 is the topology table (nvdiffrast's topology hash): built once per triangle list by
 * tsamd_antialias_topology with a workspace of tsamd_antialias_topology_workspace_bytes(n_triangles).
 * color_dev / out_dev / grad_*: [batch, height, width, n_channels] f32.  The backward recomputes the analysis (no state is
 * kept between the calls); grad_color_dev and grad_pos_dev ([batch, n_vertices, 4], zero-filled first) may each be NULL.
 * prepared_dev is OPTIONAL (NULL: everything is computed per use, identical results): tsamd_antialias_prepare fills it
 * (tsamd_antialias_prepared_bytes bytes) from the same rast_dev / pos_clip_dev / tri_dev / edge_partner_dev / sizes with (1) the
 * window coordinates of every (view, vertex) in float64, (2) a 2-bit-per-pixel mask of the pixel pairs with two different
 * triangle ids, (3) per (view, triangle) which of its edges can blend at all (no partner, or a fold).  One prepared buffer
 * serves the forward and the backward call: the image is scanned once instead of twice, the analysis of a pair on an
 * interior triangle boundary ends at one byte, and no float64 division is left in it. */
int64_t tsamd_antialias_topology_workspace_bytes(int64_t n_triangles);
int tsamd_antialias_topology(const int32_t *tri_dev, int64_t n_triangles, void *workspace_dev, int32_t *edge_partner_dev, void *stream);
int64_t tsamd_antialias_prepared_bytes(int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width);
/* pair_masks_dev: tsamd_rasterize's by-product for the SAME rast image, or NULL (rast_dev is scanned) */
int tsamd_antialias_prepare(const float *rast_dev, const float *pos_clip_dev, const int32_t *tri_dev, const int32_t *edge_partner_dev,
                            const void *pair_masks_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                            void *prepared_dev, void *stream);
int tsamd_antialias(const float *color_dev, const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev,
                    const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width, int32_t n_channels, float *out_dev,
                    void *stream);
int tsamd_antialias_backward(const float *color_dev, const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev,
                             const int32_t *tri_dev, const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                             int32_t n_channels, const float *grad_out_dev, float pos_gradient_boost, float *grad_color_dev, float *grad_pos_dev,
                             void *stream);

/* The alpha stage (the reference's trainer.py fits the geometry with only_alpha=True: loss = MSE(antialias(clamp(rast[..., -1:], 0, 1)))),
 * without a rast image.  With colours in {0, 1} a pair of two covered pixels blends w (1 - 1) = 0, so only pairs with exactly one
 * background pixel are analysed, and the covered pixel's triangle always wins them: results equal tsamd_antialias of the clamp image
 * up to the rounding of its float32 sums.
 * tsamd_silhouette: ids_out_dev [batch, height, width] i32 = triangle + 1, 0 on background (what tsamd_rasterize puts into rast's
 * fourth channel); alpha_out_dev [batch, height, width, 1] f32 = coverage 0 / 1 with the silhouette pixels blended (all zero without
 * triangles); cover_masks_out_dev (tsamd_pair_masks_bytes, the layout of the pair masks): bit l = exactly one pixel of the pair is
 * background.  workspace_dev: tsamd_rasterize_workspace_bytes.  ids and cover masks are the inputs of the two backward calls.
 * tsamd_silhouette_backward: grad_pos_dev [batch, n_vertices, 4] (zero-filled first) from grad_alpha_dev [batch, height, width, 1].
 * tsamd_silhouette_mse: loss_out_dev[0] = mean((alpha - target)^2) over n floats (0 for n = 0), bitwise repeatable for the same
 * inputs; workspace_dev: tsamd_silhouette_mse_workspace_bytes(n).  tsamd_silhouette_mse_backward: the gradient of that loss of the
 * alpha image w.r.t. pos_clip without a gradient image -- alpha_dev as tsamd_silhouette wrote it, grad_loss_dev one f32 in device
 * memory (d objective / d loss).  Limits and messages are tsamd_rasterize's; nothing synchronises with the host. */
int tsamd_silhouette(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                     const int32_t *edge_partner_dev, int32_t height, int32_t width, void *workspace_dev, int32_t *ids_out_dev,
                     void *cover_masks_out_dev, float *alpha_out_dev, void *stream);
int tsamd_silhouette_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                              const int32_t *edge_partner_dev, int32_t height, int32_t width, const int32_t *ids_dev, const void *cover_masks_dev,
                              const float *grad_alpha_dev, float pos_gradient_boost, float *grad_pos_dev, void *stream);
int64_t tsamd_silhouette_mse_workspace_bytes(int64_t n);
int tsamd_silhouette_mse(const float *alpha_dev, const float *target_dev, int64_t n, void *workspace_dev, float *loss_out_dev, void *stream);
int tsamd_silhouette_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                                  const int32_t *edge_partner_dev, int32_t height, int32_t width, const int32_t *ids_dev, const void *cover_masks_dev,
                                  const float *alpha_dev, const float *target_dev, const float *grad_loss_dev, float pos_gradient_boost,
                                  float *grad_pos_dev, void *stream);

/* The depth term of the geometry stage (the reference's trainer.py with fit_depth: MSE(out["d"][..., -1] * a_ref, d_ref * a_ref), with
 * out["d"] = || interpolate(v_pos, rast) - campos ||), from the ids tsamd_silhouette leaves: no rast image, no interpolated image, no
 * gradient image.  Per pixel of view b with triangle id t: (u, v) = the clamped barycentrics tsamd_rasterize writes (the same float32
 * operations), w = (1 - u) - v, x = u a0 + v a1 + w a2 over world_pos_dev [n_vertices, 3], d = || x - campos_dev[b] || (campos_dev
 * [batch, 3]); background -- id 0, an id outside [1, n_triangles], a vertex index outside [0, n_vertices); nothing is read through
 * those -- has x = 0, so d = || campos[b] ||.  loss_out_dev[0] = mean over batch * height * width of (d m - t m)^2 for target_dev,
 * mask_dev [batch, height, width] (each product rounded to float32, squares and sums in float64 on a fixed grid: bitwise repeatable);
 * 0 without pixels or without triangles, and then nothing else is written.  depth_out_dev (optional, [batch, height, width]): d.
 * workspace_dev: tsamd_depth_mse_workspace_bytes(batch * height * width).
 * tsamd_depth_mse_backward: with g_x = grad_loss_dev[0] 2 (d m - t m) m / n (x - campos) / d (0 where d = 0), grad_world_dev
 * [n_vertices, 3] (zero-filled first) receives the (u, v, w) g_x scatter of tsamd_interpolate_backward and grad_pos_dev
 * [batch, n_vertices, 4] the gradient of (u, v) through the quotient rule of tsamd_rasterize_backward (x, y, w; the clamps treated as
 * inactive); grad_pos_dev is zero-filled first, or added to when accumulate_pos != 0 (on top of tsamd_silhouette_mse_backward's, say).
 * fp32 atomics: the last bits of the gradients vary from run to run.  Limits and messages are tsamd_rasterize's. */
int64_t tsamd_depth_mse_workspace_bytes(int64_t n);
int tsamd_depth_mse(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height, int32_t width,
                    const int32_t *ids_dev, const float *world_pos_dev, const float *campos_dev, const float *target_dev, const float *mask_dev,
                    void *workspace_dev, float *loss_out_dev, float *depth_out_dev, void *stream);
int tsamd_depth_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height,
                             int32_t width, const int32_t *ids_dev, const float *world_pos_dev, const float *campos_dev, const float *target_dev,
                             const float *mask_dev, const float *grad_loss_dev, int32_t accumulate_pos, float *grad_world_dev, float *grad_pos_dev, void *stream);

/* The normal term of the geometry stage (the reference's mesh_rasterizer.py:137-149, out["n"] = interpolate(vertex normals * [1, 1, -1],
 * rast), under a masked MSE), from the ids tsamd_silhouette leaves: no rast image, no interpolated image, no gradient image.  attr_dev
 * [n_vertices, 3] is any 3-channel vertex attribute.  Per pixel of view b with triangle id t: (u, v) = the clamped barycentrics
 * tsamd_rasterize writes (the same float32 operations), w = (1 - u) - v, n_c = u a0_c + v a1_c + w a2_c; background -- id 0, an id
 * outside [1, n_triangles], a vertex index outside [0, n_vertices); nothing is read through those -- has n = 0.  loss_out_dev[0] = mean
 * over batch * height * width * 3 of (n_c m - t_c m)^2 for target_dev [batch, height, width, 3] and mask_dev [batch, height, width],
 * broadcast over the channels (each product rounded to float32, squares and sums in float64 on a fixed grid: bitwise repeatable); 0
 * without pixels or without triangles, and then nothing else is written.  normal_out_dev (optional, [batch, height, width, 3]): n.
 * workspace_dev: tsamd_normal_mse_workspace_bytes(batch * height * width).
 * tsamd_normal_mse_backward: with g_c = grad_loss_dev[0] 2 (n_c m - t_c m) m / (3 batch height width), grad_attr_dev [n_vertices, 3]
 * (zero-filled first) receives the (u, v, w) g scatter of tsamd_interpolate_backward and grad_pos_dev [batch, n_vertices, 4] the gradient
 * of (u, v) through the quotient rule of tsamd_rasterize_backward (x, y, w; the clamps treated as inactive); grad_pos_dev is zero-filled
 * first, or added to when accumulate_pos != 0 (on top of tsamd_silhouette_mse_backward's and tsamd_depth_mse_backward's, say).
 * Background and masked-out pixels contribute nothing.  fp32 atomics: the last bits of the gradients vary from run to run.  Limits and
 * messages are tsamd_rasterize's. */
int64_t tsamd_normal_mse_workspace_bytes(int64_t n);
int tsamd_normal_mse(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height, int32_t width,
                     const int32_t *ids_dev, const float *attr_dev, const float *target_dev, const float *mask_dev, void *workspace_dev, float *loss_out_dev,
                     float *normal_out_dev, void *stream);
int tsamd_normal_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height,
                              int32_t width, const int32_t *ids_dev, const float *attr_dev, const float *target_dev, const float *mask_dev,
                              const float *grad_loss_dev, int32_t accumulate_pos, float *grad_attr_dev, float *grad_pos_dev, void *stream);

/* The texture stage's image side under frozen geometry and fixed views (the reference's trainer.py with optimize_geo = False:
 * loss = L1(antialias(lerp(background, scatter(color), mask))[..., :3], target[..., :3])).  Which triangle wins a pixel pair, which
 * silhouette edge crosses between the two centres and the weight |t - 1/2| depend on rast / pos_clip only, so antialiasing is a
 * fixed sparse linear operator on the per-pixel colours: out_p = c_p + sum_e w_e (c_src(e) - c_p) over the blends e with
 * destination p, c_p = color[pix_point[p]] on foreground, background[p] elsewhere.  Its transpose is its whole backward.
 *
 * tsamd_shade_plan_count / _fill extract the blends of tsamd_antialias on (rast_dev, pos_clip_dev, prepared_dev of
 * tsamd_antialias_prepare -- required) as records: _count writes counts_out_dev[2 pixel + axis] = blends of the pixel's pair with
 * its right (axis 0) / upper (axis 1) neighbour; the caller scans the counts exclusively into offsets_dev and _fill stores
 * (destination pixel, source pixel, weight = f32(|t - 1/2|)) of every pair from its offset on, pixel indices batch-wide: the
 * order of the records is the order of the pair slots.  batch * height * width must stay below 2^30 and n_blends below 2^31.
 *
 * tsamd_blend_plan names the device arrays the hot calls read (all i32 unless noted):
 *   pix_point [pixels]    index of the pixel's row in color_dev, -1 on background      pix_dst [pixels]   destination slot or -1
 *   dst_ptr [n_dst + 1]   record range of a destination slot in the arrays grouped by destination:
 *                         dst_src_pix (source pixel), dst_src_point (pix_point of the source pixel), dst_weight (f32)
 *   src_ptr [n_src + 1]   record range of a source slot in the arrays grouped by source:
 *                         src_dst_pix (destination pixel), src_dst_slot (its destination slot), src_weight (f32)
 *   point_pix / point_dst / point_src [n_points]   pixel, destination slot or -1, source slot or -1 of a point
 * Every index is checked against its array before use (an index out of range reads as background / contributes nothing).
 *
 * tsamd_shade: out_dev [batch, height, width, 3] f32 from color_dev [n_points, 3] and background_dev [batch, height, width, 3],
 * float32, out = ((c_p + w_0 (c_src0 - c_p)) + w_1 (c_src1 - c_p)) + ... in the order of the destination's records, every
 * difference, product and sum rounded on its own.  tsamd_shade_backward: grad_color_dev [n_points, 3] from the gradient image,
 * grad_color[k] = (g_p (1 - ((w_0 + w_1) + ...)) + w'_0 g_dst0) + w'_1 g_dst1 ..., w over the records with destination p, w' over
 * those with source p; no atomics.
 * tsamd_shade_l1: loss_out_dev[0] = mean |out[..., c] - target[..., c]|, c < 3 (0 without pixels), target_dev [batch, height, width,
 * target_channels] with target_channels 3 or 4; float32 difference, float64 absolute values and sums in a fixed order: bitwise
 * repeatable.  image_out_dev (optional) receives out; point_sign_out_dev [n_points, 3] and dst_sign_out_dev [n_dst, 3] (optional,
 * both or neither) receive sign(out - target) in {-1, 0, 1} per point and per destination slot for tsamd_shade_l1_backward, which
 * forms g = sign * (grad_loss_dev[0] / (3 pixels)) and applies the formula of tsamd_shade_backward.  workspace_dev:
 * tsamd_shade_l1_workspace_bytes(pixels).  Nothing synchronises with the host. */
typedef struct tsamd_blend_plan {
    int32_t struct_size; /* sizeof(tsamd_blend_plan) */
    int32_t height, width;
    int32_t reserved;
    int64_t batch, n_points, n_blends, n_dst, n_src;
    const int32_t *pix_point_dev, *pix_dst_dev;
    const int32_t *dst_ptr_dev, *dst_src_pix_dev, *dst_src_point_dev;
    const float *dst_weight_dev;
    const int32_t *src_ptr_dev, *src_dst_pix_dev, *src_dst_slot_dev;
    const float *src_weight_dev;
    const int32_t *point_pix_dev, *point_dst_dev, *point_src_dev;
} tsamd_blend_plan;

int tsamd_shade_plan_count(const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev,
                           const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                           int32_t *counts_out_dev, void *stream);
int tsamd_shade_plan_fill(const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev,
                          const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                          const int32_t *offsets_dev, int64_t n_blends, int32_t *dst_out_dev, int32_t *src_out_dev, float *weight_out_dev, void *stream);
int tsamd_shade(const tsamd_blend_plan *plan, const float *color_dev, const float *background_dev, float *out_dev, void *stream);
int tsamd_shade_backward(const tsamd_blend_plan *plan, const float *grad_out_dev, float *grad_color_dev, void *stream);
int64_t tsamd_shade_l1_workspace_bytes(int64_t pixels);
int tsamd_shade_l1(const tsamd_blend_plan *plan, const float *color_dev, const float *background_dev, const float *target_dev, int32_t target_channels,
                   void *workspace_dev, float *loss_out_dev, float *image_out_dev, float *point_sign_out_dev, float *dst_sign_out_dev, void *stream);
int tsamd_shade_l1_backward(const tsamd_blend_plan *plan, const float *point_sign_dev, const float *dst_sign_dev, const float *grad_loss_dev,
                            float *grad_color_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Hash-grid encoding (the texture stage's colour field): tiny-cuda-nn's `Grid` encoding, 3-D input, trilinear,
 *   tsamd_grid_encode          <- tcnn.Encoding(3, {"otype": "HashGrid" | "DenseGrid" | "Grid", ...})(x)   models/networks.py:97-106
 *   tsamd_grid_encode_backward <- its backward w.r.t. the parameters and (optionally) x
 * Semantics (Instant-NGP, Mueller et al. 2022, as tiny-cuda-nn's published grid.h states them) are fixed by
 * tests/hashgrid_oracle.py; PARITY UNPINNED against the library itself.  Config: n_levels 1 .. 32, n_features_per_level in
 * {1, 2, 4, 8}, log2_hashmap_size 1 .. 30, base_resolution >= 1, per_level_scale >= 1, dense 0 (Hash: levels above
 * 2^log2_hashmap_size entries are hashed) or 1 (Dense: no cap).  x_dev: [n_points, 3] f32 (not clamped); params_dev:
 * [n_params] f32, level-major, n_features_per_level contiguous values per entry; out_dev / grad_out_dev: [n_points,
 * n_levels * n_features_per_level] f32, level-major columns.  params_dev, out_dev, grad_out_dev and grad_params_dev must be
 * aligned to one entry's vector (4, 8 or 16 bytes).  Stateless; the current HIP device is used.
 *
 * tsamd_grid_layout (host only): per-level first entry (offsets_out, n_levels + 1 values, the last = total entries),
 * resolution, hashed flag (1 = prime hash, 0 = dense index) and float32 scale, and the parameter count.  Each output may be NULL.
 * tsamd_grid_encode_backward ADDS dL/dparams into grad_params_dev (zero it first; NULL: not computed; a float-atomic sum,
 * not bitwise repeatable) and WRITES dL/dx into grad_x_dev ([n_points, 3], NULL: not computed).  The forward and dL/dx are
 * bitwise repeatable. */
int tsamd_grid_layout(int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                      float per_level_scale, int32_t dense, int64_t *offsets_out, int32_t *resolution_out, int32_t *hashed_out,
                      float *scale_out, int64_t *n_params_out);
int tsamd_grid_encode(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels, int32_t n_features_per_level,
                      int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense, float *out_dev,
                      void *stream);
int tsamd_grid_encode_backward(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels,
                               int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                               float per_level_scale, int32_t dense, const float *grad_out_dev, float *grad_params_dev,
                               float *grad_x_dev, void *stream);

/* The sorted backward: the same gradients as tsamd_grid_encode_backward with dL/dparams summed without float atomics (per
 * level: one (entry, source) record per point and corner, a stable radix sort by entry, a segmented sum in a fixed order).
 *   Repeatability: for given x, grad_out, config and initial contents of grad_params_dev, the resulting grad_params_dev is one
 *     bit pattern: the same across repeated calls, on any stream, whatever else the device is running, whatever the workspace
 *     held on entry and wherever the workspace lies.  It is NOT promised to be invariant under a permutation of the points.
 *   Accuracy: |g - ref| <= 2e-5 * sum|adds| + 1e-6 per value against the float64 oracle (tests/hashgrid_oracle.py), the atomic
 *     route's bound.
 *   Like tsamd_grid_encode_backward it ADDS into grad_params_dev (zero it first) and WRITES grad_x_dev (the same kernel: the
 *     same bits).  grad_params_dev == NULL: dL/dx only, no workspace needed.
 * The points go through in chunks of tsamd_grid_sorted_chunk_points() (a power of two), in order, on `stream`; the call makes no
 * allocation and no host synchronisation.  workspace_dev: 256-byte aligned, at least
 * tsamd_grid_backward_sorted_workspace_bytes(n_points, config) bytes (a function of n_points and the config only,
 * non-decreasing in n_points and constant from one chunk on); its contents on entry do not matter.  A null, misaligned or
 * too-small workspace is TSAMD_ERR_INVALID_ARGUMENT before anything is launched. */
int64_t tsamd_grid_sorted_chunk_points(void);
int tsamd_grid_backward_sorted_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                                               int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                               int32_t dense, int64_t *bytes_out);
int tsamd_grid_encode_backward_sorted(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels,
                                      int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                                      float per_level_scale, int32_t dense, const float *grad_out_dev, float *grad_params_dev,
                                      float *grad_x_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

/* The planned backward: the sorted backward's dL/dparams for a FROZEN point set, with the sort done once.
 * tsamd_grid_plan_build sorts the points' (entry, source) records as the sorted backward does and keeps, per chunk and level,
 * the 4-byte source (8 * point_in_chunk + corner) of every record in sorted order: [chunk][level][8 * points_in_chunk] uint32,
 * tsamd_grid_plan_bytes(n_points, config) bytes (>= n_points * 8 * n_levels * 4; a function of n_points and the config only,
 * non-decreasing in n_points).  tsamd_grid_encode_backward_planned is then only the segmented sum over that stored order and
 * its fold, every level of a chunk in one launch: no sort, no float atomics.
 *   Same bits: for the same x, grad_out, config and initial contents of grad_params_dev, the result is bitwise equal to
 *     tsamd_grid_encode_backward_sorted's; its repeatability and accuracy clauses carry over unchanged.
 *   Placement: the result does not depend on where the plan or the workspace lie, nor on what the workspace (or, for the build,
 *     the plan buffer) held on entry; nothing is written outside them and grad_params_dev.
 *   Memory safety: any byte pattern in the plan keeps every access in bounds (a record is followed only while its source is
 *     inside the chunk; its entry is recomputed from x_dev) -- a stale or foreign plan gives wrong numbers, nothing worse.
 *   Caller's contract: x_dev, n_points and the config of a backward are those the plan was built with.
 *   It ADDS into grad_params_dev (zero it first).  There is no dL/dx with a plan: a planned point set is frozen.
 * Both calls run on `stream`, in chunks of tsamd_grid_sorted_chunk_points(), and make no allocation and no host
 * synchronisation.  plan_dev and workspace_dev: 256-byte aligned.  The build's workspace is
 * tsamd_grid_backward_sorted_workspace_bytes(n_points, config) bytes; the backward's is
 * tsamd_grid_backward_planned_workspace_bytes(n_points, config) bytes (constant from one chunk on).  A null, misaligned or
 * too-small plan or workspace, a null grad_out_dev / grad_params_dev, n_points < 0 or an unsupported config is
 * TSAMD_ERR_INVALID_ARGUMENT before anything is launched; n_points == 0 succeeds without touching a device. */
int tsamd_grid_plan_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                          int32_t base_resolution, float per_level_scale, int32_t dense, int64_t *bytes_out);
int tsamd_grid_plan_build(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                          int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense, void *plan_dev,
                          int64_t plan_bytes, void *workspace_dev, int64_t workspace_bytes, void *stream);
int tsamd_grid_backward_planned_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                                                int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                                int32_t dense, int64_t *bytes_out);
int tsamd_grid_encode_backward_planned(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                                       int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                                       const float *grad_out_dev, float *grad_params_dev, const void *plan_dev, int64_t plan_bytes,
                                       void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fully fused MLP (the texture stage's colour MLP when its config names a tcnn network): tiny-cuda-nn's FullyFusedMLP,
 *   tsamd_mlp_forward  <- tcnn.Network(n_in, n_out, {"otype": "FullyFusedMLP" | "CutlassMLP" | "MLP", ...})(x)   models/networks.py:314-321
 *   tsamd_mlp_backward <- its backward w.r.t. the parameters and (optionally) x
 * Semantics are fixed by tests/mlp_oracle.py; PARITY UNPINNED against the library itself.  Config: n_neurons W in {16, 32,
 * 64, 128}, n_hidden_layers L 1 .. 8, n_input_dims 1 .. 256, n_output_dims 1 .. 64, activation NONE or RELU, output_activation
 * NONE or SIGMOID.  Bias-free; in_w = next_multiple(n_input_dims, 16), out_w = next_multiple(n_output_dims, 16).  params_dev:
 * [n_params] f32 = L + 1 row-major [out, in] matrices one after another: [W, in_w], (L - 1) x [W, W], [out_w, W].  Padded input
 * columns read 1.0 (the first matrix's padded columns act as a bias); padded output rows are computed and discarded.
 * Forward per row: a0 = fp16(x); a_l = fp16(act(sum_k fp16(W_l[j,k]) a_{l-1}[k])) with fp32 sums; y = out_act(sum_k
 * fp16(W_out[j,k]) a_L[k]) in fp32, returned as f32 (tiny-cuda-nn returns half).  Backward with the loss scale S = 128 of
 * tiny-cuda-nn's torch binding: delta_out = fp16(S dy out_act'(z)) (S dy above 65504 is not guarded), delta_l =
 * fp16((sum_j fp16(W_{l+1}[j,k]) delta_{l+1}[j]) act'(a_l)) with ReLU' = (a_l > 0) on the stored fp16 a_l,
 * dW_l = (sum over rows of delta_l (x) a_{l-1}) / S in fp32, dx = (sum_j fp16(W_1[j,k]) delta_1[j]) / S.  x_dev: [n_rows,
 * n_input_dims] f32; y_dev / grad_y_dev: [n_rows, n_output_dims] f32.  Stateless and stream-ordered; the current HIP device is
 * used; nothing is allocated and the host is never synchronised.  n_rows = 0 is a no-op that needs no device.
 *
 * tsamd_mlp_layout (host only): n_params, in_w and out_w (each output may be NULL).
 * tsamd_mlp_workspace_bytes (host only): the workspace tsamd_mlp_backward needs for n_rows rows when it computes grad_params
 * (one partial per workgroup, summed in a fixed order); -1 on an invalid config.
 * tsamd_mlp_backward WRITES dL/dparams into grad_params_dev ([n_params], NULL: not computed) and dL/dx into grad_x_dev
 * ([n_rows, n_input_dims], NULL: not computed).  No float atomics: y, dx and dW are bitwise repeatable for a given n_rows. */
#define TSAMD_MLP_ACT_NONE 0
#define TSAMD_MLP_ACT_RELU 1
#define TSAMD_MLP_ACT_SIGMOID 2
int tsamd_mlp_layout(int32_t n_input_dims, int32_t n_output_dims, int32_t n_neurons, int32_t n_hidden_layers, int32_t activation,
                     int32_t output_activation, int64_t *n_params_out, int32_t *in_width_out, int32_t *out_width_out);
int64_t tsamd_mlp_workspace_bytes(int64_t n_rows, int32_t n_input_dims, int32_t n_output_dims, int32_t n_neurons,
                                  int32_t n_hidden_layers, int32_t activation, int32_t output_activation);
int tsamd_mlp_forward(const float *x_dev, int64_t n_rows, const float *params_dev, int32_t n_input_dims, int32_t n_output_dims,
                      int32_t n_neurons, int32_t n_hidden_layers, int32_t activation, int32_t output_activation, float *y_dev,
                      void *stream);
int tsamd_mlp_backward(const float *x_dev, int64_t n_rows, const float *params_dev, int32_t n_input_dims, int32_t n_output_dims,
                       int32_t n_neurons, int32_t n_hidden_layers, int32_t activation, int32_t output_activation,
                       const float *grad_y_dev, float *grad_params_dev, float *grad_x_dev, void *workspace_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Texture atlas and texture sampling: the last step of the texture stage, a textured mesh,
 *   tsamd_atlas_bake_positions <- what renderer.export(path, "material") bakes (renderers/mesh_rasterizer.py:165; the reference
 *                                 goes through trimesh / pymeshlab / xatlas, none of which is used here)
 *   tsamd_texture              <- dr.texture(tex, uv, filter_mode, boundary_mode) of nvdiffrast, without mipmaps and cube maps
 * Semantics are fixed by tests/atlas_oracle.py and tests/texture_oracle.py; PARITY UNPINNED against pymeshlab's and
 * nvdiffrast's own results.  Stateless; the caller owns all buffers and the current HIP device is used.
 *
 * The atlas is closed form, no packer.  T triangles in a square texture of R texels: n = ceil(sqrt(ceil(T / 2))) cells per
 * row, c = R / n (integer) texels per cell, legs of L = c - 5 texels; c >= 6 is required.  Cell k = t / 2 has its origin at
 * ((k % n) c, (k / n) c) and holds triangle 2 k as half A and 2 k + 1 as half B, two mirrored right triangles of the same
 * orientation.  Texel (i, j) is column i, row j, its centre (i + 0.5, j + 0.5); uv = texel / R, no flip.  Corners relative
 * to the cell origin, A: (1.5, 1.5), (1.5 + L, 1.5), (1.5, 1.5 + L); B: (c - 1.5, c - 1.5), (c - 1.5 - L, c - 1.5),
 * (c - 1.5, c - 1.5 - L).  Ownership with local i, j in 0 .. c - 1: A owns i + j <= L + 3, B owns i + j >= 2 c - L - 5, the
 * band between them, the texels outside the n c square and the halves of triangles >= T are unowned.  Every bilinear tap of
 * non-zero weight of a point inside a UV triangle is a texel that triangle owns.  Barycentrics of an owned texel, extrapolated
 * into the gutter so that bilinear sampling reproduces a linear function up to the edge: A: b1 = (i - 1) / L, b2 = (j - 1) / L;
 * B: b1 = (c - 2 - i) / L, b2 = (c - 2 - j) / L; b0 = 1 - b1 - b2.
 *
 * tsamd_atlas_layout (host only): n, c and L.  The outputs (each may be NULL) are written whenever n_triangles is 1 .. 2^31
 * and texture_res 1 .. 32768, also when c < 6 makes the call fail with TSAMD_ERR_INVALID_ARGUMENT: 6 n is then the smallest
 * workable resolution, and the error text names it.
 * tsamd_atlas_bake_positions: one lane per texel; positions_out_dev [R, R, 3] f32 = b0 v0 + b1 v1 + b2 v2 of the owning
 * triangle in fp32, owner_out_dev [R, R] i32 = its index; an unowned texel gets owner -1 and position 0.  A triangle with a
 * vertex index outside [0, n_vertices) is unowned; nothing is read or written out of bounds.  v_pos_dev: [n_vertices, 3] f32;
 * tri_dev: [n_triangles, 3] i32. */
int tsamd_atlas_layout(int64_t n_triangles, int32_t texture_res, int32_t *cells_per_row_out, int32_t *cell_out, int32_t *leg_out);
int tsamd_atlas_bake_positions(const float *v_pos_dev, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                               int32_t texture_res, float *positions_out_dev, int32_t *owner_out_dev, void *stream);

/* tex_dev: [tex_batch (1 or batch), tex_height, tex_width, n_channels] f32; uv_dev: [batch, height, width, 2] f32, 8-byte
 * aligned; out_dev / grad_out_dev: [batch, height, width, n_channels] f32.  tex_height, tex_width 1 .. 32768.
 * LINEAR: x = u W - 0.5, y = v H - 0.5 (a rounded product, then the difference; no flip), taps at floor(x), floor(x) + 1 and
 * likewise in y, weights from the fractional parts.  NEAREST: the texel floor(u W), floor(v H).  WRAP reduces tap indices
 * modulo the size (a true modulo: negative indices work), CLAMP clamps them, ZERO gives out-of-range taps the value 0.
 * Indices are formed from coordinates kept within +-1e9; a non-finite uv gives a non-finite output, never an access out of
 * bounds.
 * tsamd_texture_backward: grad_tex_dev (tex's shape; NULL: not computed) is zero-filled by the call and accumulated with
 * float atomics, summed over the batch when tex_batch is 1: not bitwise repeatable.  grad_uv_dev ([batch, height, width, 2],
 * 8-byte aligned; NULL: not computed; LINEAR only, with NEAREST it must be NULL) is written: dL/du = W sum_c g_c ((t10 - t00)
 * (1 - fy) + (t11 - t01) fy) and likewise dL/dv with H, from the taps actually used, so two clamped taps that coincide give 0.
 * tex_dev may be NULL when grad_uv_dev is. */
#define TSAMD_TEX_FILTER_NEAREST 0
#define TSAMD_TEX_FILTER_LINEAR 1
#define TSAMD_TEX_BOUNDARY_WRAP 0
#define TSAMD_TEX_BOUNDARY_CLAMP 1
#define TSAMD_TEX_BOUNDARY_ZERO 2
int tsamd_texture(const float *tex_dev, int64_t tex_batch, int32_t tex_height, int32_t tex_width, int32_t n_channels,
                  const float *uv_dev, int64_t batch, int32_t height, int32_t width, int32_t filter_mode, int32_t boundary_mode,
                  float *out_dev, void *stream);
int tsamd_texture_backward(const float *tex_dev, int64_t tex_batch, int32_t tex_height, int32_t tex_width, int32_t n_channels,
                           const float *uv_dev, int64_t batch, int32_t height, int32_t width, int32_t filter_mode,
                           int32_t boundary_mode, const float *grad_out_dev, float *grad_tex_dev, float *grad_uv_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Sphere initialisation: silhouettes -> visual hull -> exact squared distance transform -> greedy ball cover, the job of the
 * reference's data/generate_init_spheres.py (whose skeleton + MILP selection is NOT rebuilt: DESIGN.md).  Semantics are fixed by
 * tests/spheres_init_oracle.py and are stated in integers, separately rounded float32 operations and single double products, so
 * the results are bitwise repeatable.  Stateless; the caller owns all buffers, workspaces included; the current HIP device is
 * used and nothing synchronises the host.
 *
 * The grid: G = grid voxels per axis, 1 .. 512, over the cube [lo, hi]^3; h = (hi - lo) / G; voxel (i, j, k) has the flat
 * index (i G + j) G + k and the centre float32(lo + (index + 0.5) h) per axis (double arithmetic, rounded once).
 *
 * tsamd_hull_carve: alpha_dev [batch, height, width, channels] f32, mvp_dev [batch, 4, 4] f32 row-major (clip = mvp (x, y, z, 1)),
 * height, width 1 .. 8192 (0 only with batch 0).  bits_workspace_dev: batch x height x ceil(width / 32) u32; the call first packs
 * alpha[..., channel] > threshold into it, one bit per pixel (bit x % 32 of word x / 32 of its row).  hull_out_dev [G, G, G] u8 is
 * 1 where, for every view, with clip_r = ((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3] in float32: clip_3 > 0, nx = clip_0 /
 * clip_3 and ny = clip_1 / clip_3 have |nx| < 1 and |ny| < 1, and the pixel (min(width - 1, floor(((nx + 1) 0.5) width)), the
 * same in y with height; row 0 is ny = -1) has its bit set.  A comparison with a NaN is false.  No read leaves the image whatever
 * mvp holds.  batch 0: every voxel is inside.
 *
 * tsamd_edt_squared: mask_dev [G, G, G] u8 (non-zero = true).  d2_out_dev [G, G, G] i32 = the squared distance in voxel units from
 * each voxel to the nearest false voxel (0 where the mask is false; nothing outside the array counts as background).
 * workspace_dev: G^3 i32.  status_out_dev: one i32, 1 when the mask has a false voxel, else 0 -- d2_out_dev is then undefined.
 *
 * tsamd_greedy_cover: at most n_spheres (0 .. 2^20) times: take q = max d2 over the uncovered voxels (initially hull_dev), the
 * lowest flat index k among equals; stop when nothing is uncovered, q == 0 or double(q) hs2 < m2; record (k, q) and clear every
 * voxel v with double(D2(v, k)) <= double(q) s2, D2 the squared index distance.  The caller passes s2 = shrink^2, hs2 = (h
 * shrink)^2 and m2 = min_radius^2.  One launch per record and one more; count_out_dev (one i32) and the first count entries of
 * flat_out_dev / q_out_dev [n_spheres] i32 hold the records, uncovered_out_dev [G, G, G] u8 (may be hull_dev itself) what is left.
 * workspace_dev: 8 (n_spheres + 1) bytes, 8-byte aligned. */
int tsamd_hull_carve(const float *alpha_dev, int64_t batch, int32_t height, int32_t width, int32_t channels, int32_t channel, float threshold,
                     const float *mvp_dev, int32_t grid, double lo, double hi, uint32_t *bits_workspace_dev, uint8_t *hull_out_dev, void *stream);
int tsamd_edt_squared(const uint8_t *mask_dev, int32_t grid, int32_t *workspace_dev, int32_t *d2_out_dev, int32_t *status_out_dev, void *stream);
int tsamd_greedy_cover(const uint8_t *hull_dev, const int32_t *d2_dev, int32_t grid, int32_t n_spheres, double s2, double hs2, double m2,
                       void *workspace_dev, uint8_t *uncovered_out_dev, int32_t *flat_out_dev, int32_t *q_out_dev, int32_t *count_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Merging tet-spheres into one closed surface (the job the reference gives to TetWild, not a rebuild of it): the union field of
 * all tets on the grid above, then marching tetrahedra on its level set.  Semantics are fixed by tests/union_oracle.py: float64
 * arithmetic on float32 inputs, every multiply, add, subtract, divide and square root rounded on its own in the order written
 * there, the maximum over tets taken on integers, so the results are bitwise repeatable.  Stateless; the caller owns all buffers;
 * the current HIP device is used and nothing synchronises the host.
 *
 * The grid: as above with G = grid in 2 .. 512; a node is a voxel centre, lo + (index + 0.5) h per axis in float64 (NOT rounded
 * to float32), flat index (i G + j) G + k.
 *
 * tsamd_union_field: tet_v_dev [n_vertices, 3] f32, elem_dev [n_tets, 4] i32 (n_tets <= 2^30).  A tet (a, b, c, d) contributes
 * only if its four indices lie in [0, n_vertices), its twelve coordinates are finite and its signed volume (b - a) . ((c - a) x
 * (d - a)) is > 0 (the orientation of scenes.kuhn_ball); other tets contribute nothing and nothing is read through a bad index.
 * For each face of a contributing tet, with q, r, s its corners ordered (b, d, c), (a, c, d), (a, d, b), (a, b, c): n = (r - q) x
 * (s - q) / |.|, which points at the opposite corner, and dist(p) = (n_x (p_x - q_x) + n_y (p_y - q_y)) + n_z (p_z - q_z);
 * m_t(p) = the least of the four (taken by d < m: a NaN never replaces a number).  The tet covers the node index box, per axis,
 * [ceil((min - lo) / h - 0.5) - 1, floor((max - lo) / h - 0.5) + 1] clipped to [0, G - 1]: its bounding box dilated by one
 * node.  field_out_dev [G, G, G] f32 = the greatest m_t(p) over the contributing tets whose box holds p, rounded once to
 * float32, -0.0 stored as +0.0, -inf where no tet covers the node.  Near the union's boundary this is the signed distance to the
 * nearest face plane, positive inside.  The call fills the buffer itself (it serves as the integer image of the maximum until
 * a last pass decodes it in place).
 *
 * tsamd_surface_count / tsamd_surface_emit: field_dev [G, G, G] f32.  A node is inside iff field > level (a NaN is outside;
 * level must not be NaN).  Each cube of 2^3 neighbouring nodes is cut into the six Kuhn tets, one per axis permutation in
 * lexicographic order (axis 0 = i), with corners o, o + e_p1, o + e_p1 + e_p2, o + (1, 1, 1).  A node owns the seven edges
 * towards node + (di, dj, dk), mask m = 4 di + 2 dj + dk in 1 .. 7.  One vertex exists per owned edge whose ends both lie in the
 * grid and differ in sign, numbered in (node flat index, m) order; with a the inside end, t = (f_a - level) / (f_a - f_b) in
 * float64 (t = 0 when that is not a number in [0, 1], which takes a non-finite value at an end) and the position is p_a + t (p_b -
 * p_a) per axis, rounded once to float32.  Each tet emits 0, 1 or 2 triangles in (cube's node flat index, permutation,
 * triangle) order, wound from the permutation's parity so that normals point from inside to outside; no geometric test.
 * tsamd_surface_count writes, per node, vmask_out_dev [G^3] u8 (bit m - 1: owned edge m carries a vertex), vcount_out_dev [G^3]
 * u8 (its bit count) and tcount_out_dev [G^3] u8 (triangles of the cube at this node, 0 on the upper borders), and
 * open_out_dev (one i32): 1 when a node on the grid's border is inside, else 0 -- the surface is closed iff it is 0.
 * tsamd_surface_emit takes the EXCLUSIVE prefix sums voffset_dev / toffset_dev [G^3] i32 of the two counts and their totals
 * n_vertices / n_triangles, and writes v_out_dev [n_vertices, 3] f32 and faces_out_dev [n_triangles, 3] i32.  Nothing is read or
 * written out of bounds whatever the masks and offsets hold; both totals 0: nothing is launched. */
int tsamd_union_field(const float *tet_v_dev, int64_t n_vertices, const int32_t *elem_dev, int64_t n_tets, int32_t grid, double lo, double hi,
                      float *field_out_dev, void *stream);
int tsamd_surface_count(const float *field_dev, int32_t grid, float level, uint8_t *vmask_out_dev, uint8_t *vcount_out_dev, uint8_t *tcount_out_dev,
                        int32_t *open_out_dev, void *stream);
int tsamd_surface_emit(const float *field_dev, int32_t grid, double lo, double hi, float level, const uint8_t *vmask_dev, const int32_t *voffset_dev,
                       const int32_t *toffset_dev, int64_t n_vertices, int64_t n_triangles, float *v_out_dev, int32_t *faces_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Flood fill of the field above: connected components of its nodes, the fill of enclosed cavities and the removal of islands.
 * Semantics are fixed by tests/fill_oracle.py; everything is integer work and bitwise repeatable.  Stateless, caller-owned
 * buffers, nothing synchronises the host.
 *
 * Connectivity is the extraction's own: two nodes are adjacent iff they differ by +-[di, dj, dk] with [di, dj, dk] in {0, 1}^3 and
 * not all zero -- the seven owned Kuhn edges of a node and their reverses, 14 neighbours ([1, -1, 0] and its kin are not edges).
 * A node is inside iff field > level (a NaN is outside; level must not be NaN).  A component is a maximal set of nodes with
 * equal inside bit connected through these edges: inside and outside nodes are labelled in one pass.
 *
 * tsamd_grid_components: label_out_dev [G, G, G] i32 = the smallest flat index in the node's component, so label <= index and
 * label[label[n]] == label[n], whatever the execution order.  status_out_dev: one i32, zero-filled by the call itself; non-zero
 * afterwards means that a bounded device loop ran out of its bound (1: a find walk, 2: a union) and the labels are not to be
 * used -- every find walk and every union retry is bounded by a multiple of G^3 that a correct run cannot reach, so a logic
 * error reports here instead of hanging the device.
 *
 * tsamd_field_fill: the exterior is every outside component holding a node of the grid's border.  mode TSAMD_FILL_CAVITIES:
 * solid = every node that is not exterior (enclosed outside components become inside, islands floating in them included).
 * mode TSAMD_FILL_OUTER: of that solid, only the component with the most nodes stays (ties: the smaller label).
 * field_out_dev [G, G, G] f32, which must not be field_dev (the input is never modified): a node whose inside bit is
 * unchanged keeps its value bit for bit, an outside node that became inside reads +inf, an inside node that became outside reads
 * -inf.  A changed node has no neighbour of opposite final sign, so these values are never interpolated and the extraction of
 * the new field is a sub-mesh of the extraction of the old one.  workspace_dev: [2 G^3 + 2] i32, 8-byte aligned, contents
 * undefined before and after.  stats_out_dev: five i32, zero-filled by the call itself: the status word as above, cavities
 * (outside components not touching the border), cavity_nodes, islands (solid components dropped) and island_nodes (the last
 * two are 0 in mode TSAMD_FILL_CAVITIES). */
#define TSAMD_FILL_CAVITIES 1
#define TSAMD_FILL_OUTER 2
int tsamd_grid_components(const float *field_dev, int32_t grid, float level, int32_t *label_out_dev, int32_t *status_out_dev, void *stream);
int tsamd_field_fill(const float *field_dev, int32_t grid, float level, int32_t mode, void *workspace_dev, float *field_out_dev, int32_t *stats_out_dev,
                     void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Surface metrics: area-uniform surface samples and the nearest-point search that Chamfer distance, F-score and normal
 * consistency rest on (tssplat_amd/metrics.py).  Semantics are fixed by tests/metrics_oracle.py, in separately rounded
 * operations and integer minima and maxima: bitwise repeatable and equal to the oracle.  Stateless, caller-owned buffers,
 * nothing synchronises the host.
 *
 * tsamd_sample_surface, phase TSAMD_SAMPLE_WEIGHTS: v_dev [n_vertices, 3] f32, faces_dev [n_triangles, 3] i32.  Per triangle,
 * in float64 on the float32 corners a, b, c: n = [b - a] x [c - a], each component two rounded products and a difference,
 * w = sqrt[[nx nx + ny ny] + nz nz].  A triangle with an index outside the vertices, a coordinate that is not finite or w = 0
 * has the integer weight 0; every other one q = floor[[w / w_max] 2^32] with w_max the largest w, so 1 <= q_max = 2^32.
 * prefix_dev [n_triangles] i64 receives q (the caller turns it into its inclusive prefix sum); workspace_dev: 8 bytes, 8-byte
 * aligned.  n_samples, seed and the three outputs are not used.
 * Phase TSAMD_SAMPLE_DRAW: prefix_dev holds the inclusive prefix sum C of q with Q = C[n_triangles - 1] > 0, which is the
 * caller's to check.  With mix64[seed, c] the splitmix64 finaliser of seed + [c + 1] 0x9E3779B97F4A7C15, sample i takes
 * p = the high 64 bits of mix64[seed, 3 i] Q and the first triangle t with C[t] > p; the 24-bit integers
 * ia = mix64[seed, 3 i + 1] >> 40 and ib = mix64[seed, 3 i + 2] >> 40, both replaced by 2^24 minus themselves when
 * ia + ib > 2^24; a = ia 2^-24, b = ib 2^-24 and the point [A + a [B - A]] + b [C - A] in float32, every operation rounded
 * on its own.  points_out_dev [n_samples, 3] f32; normals_out_dev [n_samples, 3] f32 = n / w of the triangle, rounded once;
 * tri_out_dev [n_samples] i32 = t.  workspace_dev is not used.  Nothing is read out of bounds whatever prefix_dev holds (a
 * triangle that cannot be drawn gives NaN).  n_samples = 0: nothing is launched.
 *
 * tsamd_nearest_points: query_dev [n, 3] f32, ref_dev [m, 3] f32, m >= 1.  Per query the minimum over all ref points of
 * d2 = [[qx - rx]^2 + [qy - ry]^2] + [qz - rz]^2 in float32, in exactly that order, every operation rounded on its own; the lower
 * index wins a tie; a pair whose d2 is NaN is skipped; +inf is an ordinary value.  d2_out_dev [n] f32, idx_out_dev [n] i32;
 * a query with no pair left gives +inf and -1.  ref_chunks: into how many parts the ref points are split over the grid's second
 * dimension (1 .. min[m, 65535]; 0: the automatic rule that tsamd_nearest_points_info reports); the result does not depend
 * on it, bit for bit.  workspace_dev: tsamd_nearest_points_workspace_bytes[n] bytes (8 per query; -1 for an n out of range),
 * 8-byte aligned, filled by the call itself, contents undefined afterwards.  n = 0: nothing is launched.
 * tsamd_nearest_points_info: the compiled lanes per workgroup, queries per lane and ref points per LDS tile, and the chunk
 * count the automatic rule picks for n queries and m ref points; it touches no device. */
#define TSAMD_SAMPLE_WEIGHTS 0
#define TSAMD_SAMPLE_DRAW 1
int tsamd_sample_surface(int32_t phase, const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int64_t *prefix_dev,
                         void *workspace_dev, int64_t n_samples, uint64_t seed, float *points_out_dev, float *normals_out_dev, int32_t *tri_out_dev,
                         void *stream);
int64_t tsamd_nearest_points_workspace_bytes(int64_t n);
int tsamd_nearest_points_info(int64_t n, int64_t m, int32_t *block_out, int32_t *queries_per_lane_out, int32_t *ref_tile_out, int32_t *auto_chunks_out);
int tsamd_nearest_points(const float *query_dev, int64_t n, const float *ref_dev, int64_t m, int32_t ref_chunks, void *workspace_dev, float *d2_out_dev,
                         int32_t *idx_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Exact point-to-triangle search: for every query the closest triangle of a mesh, its squared distance and the closest point
 * (tssplat_amd/metrics.py: nearest_on_mesh, compare_meshes_exact).  Semantics are fixed by tests/pointmesh_oracle.py, in
 * separately rounded float64 operations and integer minima: bitwise repeatable and equal to the oracle.  Stateless, caller-owned
 * buffers, nothing synchronises the host.
 *
 * tsamd_nearest_on_mesh: query_dev [n, 3] f32, v_dev [n_vertices, 3] f32, faces_dev [n_triangles, 3] i32, n_triangles >= 1.  A
 * triangle is valid iff its indices lie in 0 .. n_vertices - 1, its nine coordinates are finite and the weight w of
 * tsamd_sample_surface is > 0; an invalid triangle is never a result and nothing is read through a bad index.  Per query P and
 * valid triangle A B C, in float64 on the float32 inputs, every operation rounded on its own, dot[u, v] = [ux vx + uy vy] + uz vz
 * (Ericson, Real-Time Collision Detection, 5.1.5):
 *   AB = B - A, AC = C - A, AP = P - A, BP = P - B, CP = P - C;
 *   d1 = dot[AB, AP], d2 = dot[AC, AP], d3 = dot[AB, BP], d4 = dot[AC, BP], d5 = dot[AB, CP], d6 = dot[AC, CP];
 *   vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6;
 * the first test that holds gives the barycentrics (a comparison with a NaN is false):
 *   d1 <= 0 and d2 <= 0: v = 0, w = 0;    d3 >= 0 and d4 <= d3: v = 1, w = 0;    vc <= 0 and d1 >= 0 and d3 <= 0: v = d1 / [d1 - d3], w = 0;
 *   d6 >= 0 and d5 <= d6: v = 0, w = 1;   vb <= 0 and d2 >= 0 and d6 <= 0: v = 0, w = d2 / [d2 - d6];
 *   va <= 0 and e >= 0 and g >= 0: w = e / [e + g], v = 1 - w;    otherwise s = [va + vb] + vc, v = vb / s, w = vc / s;
 * X = [A + AB v] + AC w per component and d2 = [[Px - Xx]^2 + [Py - Xy]^2] + [Pz - Xz]^2.  Per query the minimum over the valid
 * triangles of fl32[d2], the float64 value rounded once (an overflow to +inf is an ordinary value); the lowest triangle index wins
 * a tie; a pair whose d2 is NaN is skipped.  d2_out_dev [n] f32, tri_out_dev [n] i32, point_out_dev [n, 3] f32 (may be null: not
 * written) = the winning triangle's X rounded once; a query with no pair left gives +inf, -1 and a NaN point -- a mesh without a
 * valid triangle is not an error.  A float32 bounding-sphere test and a seed (tsamd_nearest_points over the sphere centres) decide
 * which pairs are evaluated, never the result.  ref_chunks: into how many parts the triangles are split over the grid's second
 * dimension (1 .. min[n_triangles, 65535]; 0: the automatic rule that tsamd_nearest_on_mesh_info reports); the result does not
 * depend on it, bit for bit.  workspace_dev: tsamd_nearest_on_mesh_workspace_bytes[n, n_triangles] bytes (-1 for a count out of
 * range), 16-byte aligned, filled by the call itself, contents undefined afterwards.  n = 0: nothing is launched.
 * tsamd_nearest_on_mesh_info: the compiled lanes per workgroup, queries per lane and bounding spheres per LDS tile, and the chunk
 * count the automatic rule picks for n queries and n_triangles triangles; it touches no device. */
int64_t tsamd_nearest_on_mesh_workspace_bytes(int64_t n, int64_t n_triangles);
int tsamd_nearest_on_mesh_info(int64_t n, int64_t n_triangles, int32_t *block_out, int32_t *queries_per_lane_out, int32_t *tri_tile_out,
                               int32_t *auto_chunks_out);
int tsamd_nearest_on_mesh(const float *query_dev, int64_t n, const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles,
                          int32_t ref_chunks, void *workspace_dev, float *d2_out_dev, int32_t *tri_out_dev, float *point_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Surface simplification: vertex clustering on a cube grid with quadric placement (tssplat_amd/simplify.py).  Semantics are
 * fixed by tests/simplify_oracle.py, in separately rounded float64 operations, sequential sums and integers: bitwise repeatable
 * and equal to the oracle.  Stateless, caller-owned buffers, nothing synchronises the host.  The two sorts between the stages
 * are the caller's (their keys are unique, or the sort is stable).
 *
 * Grid: C = cells (1 .. 1024) per axis over the cube [lo, hi]^3, h = [hi - lo] / C in float64, cell [i, j, k] has the key
 * [i C + j] C + k and the centre g = lo + [index + 0.5] h per axis.  T = n_triangles <= [2^31 - 1] / 3; S = 3 T record slots.
 *
 * tsamd_simplify_keys: v_dev [n_vertices, 3] f32, faces_dev [T, 3] i32.  vkey_out_dev [n_vertices] i32: -1 for a vertex with a
 * coordinate that is not finite, else its cell key with the per-axis index floor[[x - lo] / h] clamped to 0 .. C - 1.
 * state_out_dev [T] u8: 2 for a face with an index outside 0 .. n_vertices - 1 or an invalid vertex (nothing is read through a bad
 * index), 1 for a valid face whose corners share a cell, 0 for one with three distinct cells.  records_out_dev [S] i64: slot
 * 3 t + s holds [cell << 32] | t for corner s of a valid face t if no earlier corner has that cell, else INT64_MAX.
 *
 * tsamd_simplify_cells: records_dev [S] the records sorted ascending, perm_dev [S] i64 the slot each came from.  One lane per
 * run of equal cells walks it serially in record order: with n = [b - a] x [c - a] of the record's face, a' = a - g and
 * d = -[[nx a'x + ny a'y] + nz a'z], the sums of nx nx, nx ny, nx nz, ny ny, ny nz, nz nz [A], of d n [b], and for each corner of
 * the face in this cell, in corner order, of p - g [P] and of 1 [count].  m = P / count.  TSAMD_SIMPLIFY_MEAN: x = m.
 * TSAMD_SIMPLIFY_QUADRIC: tr = [A00 + A11] + A22, lam = stabilise tr, M = A + lam I, r = lam m - b, x = M^-1 r by the symmetric
 * cofactor formula in the operation order of the oracle; x = m unless tr > 0, det > 0 and x is finite.  Each x_i is then
 * clamped to [-h/2, h/2].  At the run's first record i: pos_out_dev [S, 3] f32 = g + x rounded once, head_out_dev [S] u8 = 1, or
 * 3 when the clamp changed a coordinate (0 everywhere else); run_out_dev [S] i32, by ORIGINAL slot, = i for every slot of the run
 * (-1 for an unused slot).  status_out_dev: one i32, zero-filled by the call itself; TSAMD_SIMPLIFY_STATUS_RECORDS afterwards
 * means that the records, the permutation or the keys are not what tsamd_simplify_keys and a sort make of these faces -- the
 * outputs are not to be used, and nothing was read or written out of bounds.  Every walk is bounded by S.
 *
 * tsamd_simplify_faces: tri_out_dev [T, 3] i32: for a face of state 0 its three runs, rotated, orientation kept, so that the
 * smallest comes first [runs ascend with the cell key]; -1 -1 -1 otherwise.  key_ab_out_dev / key_c_out_dev [T] i64:
 * [a << 32] | b and c of that triple, INT64_MAX otherwise -- sorting the faces stably by key_c and then stably by key_ab orders
 * them by [triple, index].
 *
 * tsamd_simplify_dedupe: order_dev [T] i64, the faces in that order.  keep_out_dev [T] u8: 1 for a survivor whose predecessor
 * in the order holds another triple, else 0; used_out_dev [S] u8: 1 at every run a kept face names, else 0; both filled by the
 * call itself.  status_out_dev as above, TSAMD_SIMPLIFY_STATUS_ORDER for an order or triple entry out of range. */
#define TSAMD_SIMPLIFY_QUADRIC 0
#define TSAMD_SIMPLIFY_MEAN 1
#define TSAMD_SIMPLIFY_STATUS_RECORDS 1
#define TSAMD_SIMPLIFY_STATUS_ORDER 2
int tsamd_simplify_keys(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t cells, double lo, double hi,
                        int32_t *vkey_out_dev, int64_t *records_out_dev, uint8_t *state_out_dev, void *stream);
int tsamd_simplify_cells(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t cells, double lo, double hi,
                         int32_t placement, double stabilise, const int32_t *vkey_dev, const int64_t *records_dev, const int64_t *perm_dev, float *pos_out_dev,
                         uint8_t *head_out_dev, int32_t *run_out_dev, int32_t *status_out_dev, void *stream);
int tsamd_simplify_faces(const int32_t *run_dev, const uint8_t *state_dev, int64_t n_triangles, int32_t *tri_out_dev, int64_t *key_ab_out_dev,
                         int64_t *key_c_out_dev, void *stream);
int tsamd_simplify_dedupe(const int32_t *tri_dev, const int64_t *order_dev, int64_t n_triangles, uint8_t *keep_out_dev, uint8_t *used_out_dev,
                          int32_t *status_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Voxelising triangle meshes: the integer winding number at the nodes of the merge's grid, and the occupancy made of it
 * (tssplat_amd/voxelize.py).  Semantics are fixed by tests/voxel_oracle.py: exact int64 predicates on a 2^-10 lattice, float64
 * operations rounded one by one, int32 sums -- bitwise repeatable and equal to the oracle.  Stateless, caller-owned buffers,
 * nothing synchronises the host.
 *
 * Grid: G = grid (1 .. 512) nodes per axis over the cube [lo, hi]^3, h = [hi - lo] / G in float64, node [i, j, k] at
 * lo + [index + 0.5] h, flat index [i G + j] G + k.  S = 2^10.  A ray axis a has the plane axes b = [a + 1] % 3, c = [a + 2] % 3.
 *
 * v_dev [n_vertices, 3] f32, faces_dev [n_triangles, 3] i32.  Per vertex and axis t = [x - lo] / h, u = floor[t S + 0.5] as an
 * integer and r = t - 0.5; a vertex is usable iff |u| <= 2^29 on all three axes (a NaN or an infinity is not).  A face with an
 * index outside 0 .. n_vertices - 1 or a corner that is not usable is invalid; nothing is read through a bad index.  On the
 * ray's plane, area = [B_b - A_b][C_c - A_c] - [B_c - A_c][C_b - A_b]; area = 0: the face is degenerate on this ray and
 * contributes nothing; sg = sign[area].  Column [p, q] sits at P = [p S + S/2, q S + S/2]; the edge function of Q -> R is
 * E = [R_b - Q_b][P_c - Q_c] - [R_c - Q_c][P_b - Q_b]; with e = sg E and d = sg [R - Q] the column is on the edge's inner side iff
 * e > 0, or e = 0 and [d_b > 0, or d_b = 0 and d_c > 0]; a face covers the columns 0 .. G - 1 for which BC, CA and AB all say so
 * (a mesh sticking out of the cube is clipped).  It then deposits -sg at slab ceil[x] clamped to 0 .. G of that column,
 * x = [[E_BC r_A + E_CA r_B] + E_AB r_C] / area in float64.  w is the inclusive prefix sum of the deposits along the ray: +1 inside
 * a closed surface whose normals point outwards.  A column is open when its G + 1 slabs do not sum to 0.
 *
 * tsamd_voxel_workspace_bytes: 6144 + 3 [G + 1] G^2 x 4 bytes (64 copies of the counts, then three rays' deposits), or -1 for a
 * grid out of range; it touches no device.  workspace_dev: 8-byte aligned, cleared by the calls themselves, contents undefined
 * afterwards; tsamd_voxel_winding and rays = 1 use only the first 6144 + [G + 1] G^2 x 4 bytes of it.
 * stats_out_dev: twelve i64, 8-byte aligned, written by the calls themselves: [0 .. 2] open columns per axis, [3] disputed,
 * [4] invalid faces, [5 .. 7] degenerate faces per axis, [8 .. 10] deposits (covered face-column pairs) per axis, [11] faces whose
 * box of candidate columns was walked by a whole wave (more than 16 columns), summed over the rays; a ray that did not run
 * leaves its entries 0.
 * tsamd_voxel_winding: w_out_dev [G, G, G] i32 in the [i, j, k] layout for every axis (0, 1 or 2).
 * tsamd_voxel_occupancy: occ_out_dev [G, G, G] u8, 1 where the rule holds for w: TSAMD_VOXEL_NONZERO w != 0, _POSITIVE w > 0, _ODD
 * w odd.  rays = 1: axis 0.  rays = 3: the majority of the three axes' bits; disputed counts the nodes at which they differ.  No w
 * is written.  n_triangles = 0: everything is 0. */
#define TSAMD_VOXEL_NONZERO 0
#define TSAMD_VOXEL_POSITIVE 1
#define TSAMD_VOXEL_ODD 2
int64_t tsamd_voxel_workspace_bytes(int32_t grid);
int tsamd_voxel_winding(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t axis,
                        void *workspace_dev, int32_t *w_out_dev, int64_t *stats_out_dev, void *stream);
int tsamd_voxel_occupancy(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t rule,
                          int32_t rays, void *workspace_dev, uint8_t *occ_out_dev, int64_t *stats_out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Mesh quality: the exact self-intersection search and the topology of a triangle mesh (tssplat_amd/quality.py).  Semantics are
 * fixed by tests/quality_oracle.py: exact int64 predicates on a 2^20 lattice, integer counts and labels, and a float64 shape
 * record whose operations are rounded one by one -- bitwise repeatable and equal to the oracle.  Stateless, caller-owned buffers.
 * Nothing synchronises the host except tsamd_quality_union.
 *
 * tsamd_quality_prepare: v_dev [n_vertices, 3] f32, faces_dev [n_triangles, 3] i32, the cube [lo, hi]^3.  With g = [2^20 - 1] /
 * [hi - lo] in float64 a coordinate x snaps to X = floor[[double[x] - lo] g + 0.5], product and sum rounded separately.  A
 * triangle is valid iff its indices lie in 0 .. n_vertices - 1, its nine coordinates are finite and every X lies in
 * 0 .. 2^20 - 1; nothing is read through a bad index.  It is degenerate iff it is valid and the integer cross product
 * [B - A] x [C - A] of its snapped corners is zero.  state_out_dev [n_triangles] u8: 0 valid, 1 degenerate, 2 invalid.
 * corners_out_dev [n_triangles, 3] u64: a corner as X | Y << 21 | Z << 42, or ~0 three times for a triangle whose state is not 0.
 * boxes_out_dev [n_triangles, 2] u64: the minimum corner of the triangle's lattice box in the same packing, then the maximum
 * corner with the bits 20, 41 and 62 set; the box [2^20 - 1, 0] for a triangle whose state is not 0.  morton_out_dev
 * [n_triangles] i64: the 60-bit Morton code of floor[[min + max] / 2] (x in the lowest bit), 2^63 - 1 where the state is not 0.
 * shape_out_dev [n_triangles, 4] f64, in float64 on the float32 corners, every operation rounded on its own, dot[d] =
 * [dx dx + dy dy] + dz dz and the cross product's components as differences of two products: dot[B - A], dot[C - B], dot[A - C],
 * dot[[B - A] x [C - A]] (four times the squared area); NaN four times for an invalid triangle.  n_triangles = 0: nothing is
 * launched.
 *
 * tsamd_quality_pairs: the outputs of tsamd_quality_prepare, in any order of the triangles as long as the three agree.
 * orient[a, b, c, d] = det[b - a, c - a, d - a] in int64 (below 3 x 2^61 in magnitude).  A segment p q pierces a triangle a b c iff
 * orient[a, b, c, p] and orient[a, b, c, q] are non-zero with opposite signs and orient[p, q, a, b], orient[p, q, b, c],
 * orient[p, q, c, a] are all > 0 or all < 0.  Two triangles i < j of state 0 are a crossing pair iff an edge of one pierces the
 * other.  Strict signs: a contact through a vertex or along an edge, a coplanar overlap, and a crossing whose piercings all pass
 * exactly through edges of the other triangle are not counted.  crossings_out_dev [n_triangles] i32: the crossing pairs a
 * triangle is in.  pairs_out_dev [max_pairs] i64 (may be null when max_pairs = 0): the keys i << 32 | j of the first max_pairs
 * pairs found, in no order; when there are more pairs than max_pairs, which ones are listed depends on timing.  stats_out_dev:
 * eight i64, 8-byte aligned, written by the call itself: [TSAMD_QUALITY_CROSSING_PAIRS], [_CROSSING_FACES] triangles in at least
 * one pair, [_INVALID_FACES], [_DEGENERATE_FACES], [_BOX_PAIRS] pairs i < j of state 0 whose closed lattice boxes overlap,
 * [_LISTED_PAIRS] = min[crossing pairs, max_pairs], [_TILE_VISITS] tiles loaded summed over the workgroups, [7] zero.
 * tile_boxes_dev: null, or a workspace of 16 bytes per tile of the size tsamd_quality_info reports, 8-byte aligned: the call
 * then writes every tile's box there and skips the pairs of a wave and a tile whose boxes are apart.  That decides which pairs
 * are evaluated, never the result: every output but [_TILE_VISITS] is the same, bit for bit.  n_triangles = 0: the stats are
 * zeroed.
 * tsamd_quality_info: the compiled triangles per workgroup, triangles per LDS tile and queue entries per wave; it touches no
 * device.
 *
 * Topology.  Half-edge 3 t + k runs from faces[t, k] to faces[t, [k + 1] % 3]; corner 3 t + k sits at faces[t, k].
 * tsamd_quality_edges: per half-edge of a triangle whose state is not 2 and whose indices are in range, und_keys_out_dev
 * [3 n_triangles] i64 = min << 32 | max of its ends, dir_keys_out_dev = from << 32 | to, vertex_pairs_out_dev [3 n_triangles, 2]
 * i32 = its ends; for any other half-edge 2^63 - 1, 2^63 - 1 and [-1, -1].  referenced_out_dev [n_vertices] u8: 1 for the
 * vertices of those triangles, else 0.
 * tsamd_quality_fan_pairs: sorted_keys_dev [3 n_triangles] i64 the undirected keys in ascending order and order_dev
 * [3 n_triangles] i64 the half-edge each came from.  corner_pairs_out_dev [3 n_triangles, 2, 2] i32: for a position whose key
 * equals the one before and is not 2^63 - 1, with h1 the half-edge before and h2 this one, for each end x of h1 the pair of h1's
 * corner at x and h2's corner at x (h2's first corner if that sits at x, else its second); [-1, -1] twice elsewhere.
 * tsamd_quality_union: labels_out_dev [n] i32 = the lowest index of the class of each of n elements under the pairs pairs_dev
 * [n_pairs, 2] i32 (a pair with an index outside 0 .. n - 1 is skipped).  Rounds of hooking the higher of two labels to the lower
 * with an integer atomicMin and of pointer jumping; after each round the host reads one flag back, so this call SYNCHRONISES the
 * host with the stream.  It never spins: past n + 1 rounds, which a correct build cannot need, it returns TSAMD_ERR_HIP.
 * workspace_dev: 4 bytes, 4-byte aligned.  rounds_out (host, may be null): the rounds run.  The labels are a function of the
 * pairs alone. */
#define TSAMD_QUALITY_CROSSING_PAIRS 0
#define TSAMD_QUALITY_CROSSING_FACES 1
#define TSAMD_QUALITY_INVALID_FACES 2
#define TSAMD_QUALITY_DEGENERATE_FACES 3
#define TSAMD_QUALITY_BOX_PAIRS 4
#define TSAMD_QUALITY_LISTED_PAIRS 5
#define TSAMD_QUALITY_TILE_VISITS 6
int tsamd_quality_info(int32_t *block_out, int32_t *tile_out, int32_t *queue_out);
int tsamd_quality_prepare(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, double lo, double hi, uint64_t *corners_out_dev,
                          uint64_t *boxes_out_dev, uint8_t *state_out_dev, double *shape_out_dev, int64_t *morton_out_dev, void *stream);
int tsamd_quality_pairs(const uint64_t *corners_dev, const uint64_t *boxes_dev, const uint8_t *state_dev, int64_t n_triangles, uint64_t *tile_boxes_dev,
                        int64_t max_pairs, int32_t *crossings_out_dev, int64_t *pairs_out_dev, int64_t *stats_out_dev, void *stream);
int tsamd_quality_edges(const int32_t *faces_dev, const uint8_t *state_dev, int64_t n_triangles, int64_t n_vertices, int64_t *und_keys_out_dev,
                        int64_t *dir_keys_out_dev, int32_t *vertex_pairs_out_dev, uint8_t *referenced_out_dev, void *stream);
int tsamd_quality_fan_pairs(const int32_t *faces_dev, int64_t n_triangles, const int64_t *sorted_keys_dev, const int64_t *order_dev,
                            int32_t *corner_pairs_out_dev, void *stream);
int tsamd_quality_union(const int32_t *pairs_dev, int64_t n_pairs, int32_t *labels_out_dev, int64_t n, void *workspace_dev, int64_t *rounds_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Smoothing a triangle surface without touching its faces: Taubin's lambda | mu filter and tangential relaxation on the
 * umbrella operator (tssplat_amd/smooth.py).  Semantics are fixed by tests/smooth_oracle.py: float64 operations rounded one by
 * one, sums in ascending row order, no float atomics -- bitwise repeatable and equal to the oracle.  Stateless, caller-owned
 * buffers, nothing synchronises the host.
 *
 * A face is valid iff its three indices lie in 0 .. n_vertices - 1 and are pairwise distinct; nothing else contributes.
 * tsamd_smooth_keys: faces_dev [n_triangles, 3] i32 (at most 357913940 faces).  valid_out_dev [n_triangles] u8; edge_keys_out_dev
 * [6 n_triangles] i64: src << 32 | dst for both directions of the face's three edges; face_keys_out_dev [3 n_triangles] i64:
 * vertex << 32 | t per corner; 2^63 - 1 throughout for an invalid face.  The caller sorts both arrays.
 * tsamd_smooth_rows: sorted_keys_dev [n_keys] i64, the edge keys ascending.  head_out_dev [n_keys] u8: 1 at the first position
 * of every run of equal keys that is not 2^63 - 1 -- one neighbour; the heads in order are the rows of the adjacency, by source
 * and then by neighbour.  The run's length is the number of valid faces at that edge; irregular_out_dev [n_vertices] u8, filled
 * by the call: 1 for a vertex that is the source of a run whose length is not two (the opposite run marks the other end).
 *
 * tsamd_smooth_mesh names the connectivity (all i32): offsets [n_vertices + 1] and neighbours [n_neighbours], the rows in
 * ascending order; face_offsets [n_vertices + 1] and faces_of [n_face_entries], a vertex's valid faces in ascending order, and
 * faces [n_triangles, 3] -- these three are read in tangential mode only and may be null otherwise.  No entry is trusted: a row
 * that leaves its array, a neighbour outside 0 .. n_vertices - 1 or a face outside 0 .. n_triangles - 1 holds the vertex.
 * tsamd_smooth_classify: v_dev [n_vertices, 3] f32, irregular_dev [n_vertices] u8, pinned_dev [n_vertices] u8 or null.
 * class_out_dev [n_vertices] u8, the first that applies: TSAMD_SMOOTH_HELD_OTHER a coordinate that is not finite, no neighbour, or
 * a neighbour with a coordinate that is not finite; _HELD_PINNED; _HELD_IRREGULAR (boundary = TSAMD_SMOOTH_BOUNDARY_FIXED only);
 * else TSAMD_SMOOTH_MOVES.
 *
 * State: n_vertices records of stride float64, x y z first; stride 3 (8-byte aligned) or 4 (32-byte aligned, the fourth is
 * written as 0).  tsamd_smooth_step: one half-step from src_dev to dst_dev, which must be another buffer.  For a vertex that moves,
 * L = S / double[deg] - p with S the sum of its neighbours' records in row order from 0.0, per component, and d = coef L.
 * TSAMD_SMOOTH_TAUBIN: q = p + d.  TSAMD_SMOOTH_TANGENTIAL: n = the sum over its faces, in list order from 0.0, of
 * [p_b - p_a] x [p_c - p_a] (each component a difference of two products); nn = [nx nx + ny ny] + nz nz; if nn > 0,
 * s = [[dx nx + dy ny] + dz nz] / nn and q = p + [d - n s], else q = p.  v0_dev [n_vertices, 3] f32 or null: when given, each
 * coordinate of q is then clamped into [double[v0] - max_move, double[v0] + max_move] (max_move finite, >= 0; a NaN passes
 * through).  Every other vertex is copied, so dst_dev is complete.
 * tsamd_smooth_run: `iterations` (0 .. 4096) iterations between state_a_dev, which holds the start, and state_b_dev: the
 * half-step lam and, in Taubin mode, the half-step mu, each reading the result of the one before; a half-step whose coefficient
 * is exactly 0 is skipped.  *result_in_b_out (host): 1 when the result is in state_b_dev, 0 when in state_a_dev. */
#define TSAMD_SMOOTH_TAUBIN 0
#define TSAMD_SMOOTH_TANGENTIAL 1
#define TSAMD_SMOOTH_BOUNDARY_FIXED 0
#define TSAMD_SMOOTH_BOUNDARY_FREE 1
#define TSAMD_SMOOTH_MOVES 0
#define TSAMD_SMOOTH_HELD_OTHER 1
#define TSAMD_SMOOTH_HELD_PINNED 2
#define TSAMD_SMOOTH_HELD_IRREGULAR 3
typedef struct tsamd_smooth_mesh {
    int32_t struct_size; /* sizeof(tsamd_smooth_mesh) */
    int32_t reserved;
    int64_t n_vertices, n_triangles, n_neighbours, n_face_entries;
    const int32_t *offsets_dev, *neighbours_dev;
    const int32_t *face_offsets_dev, *faces_of_dev, *faces_dev;
} tsamd_smooth_mesh;

int tsamd_smooth_keys(const int32_t *faces_dev, int64_t n_triangles, int64_t n_vertices, uint8_t *valid_out_dev, int64_t *edge_keys_out_dev,
                      int64_t *face_keys_out_dev, void *stream);
int tsamd_smooth_rows(const int64_t *sorted_keys_dev, int64_t n_keys, int64_t n_vertices, uint8_t *head_out_dev, uint8_t *irregular_out_dev, void *stream);
int tsamd_smooth_classify(const float *v_dev, const tsamd_smooth_mesh *mesh, const uint8_t *irregular_dev, const uint8_t *pinned_dev, int32_t boundary,
                          uint8_t *class_out_dev, void *stream);
int tsamd_smooth_step(const double *src_dev, double *dst_dev, int32_t stride, const tsamd_smooth_mesh *mesh, const uint8_t *class_dev, int32_t mode, double coef,
                      const float *v0_dev, double max_move, void *stream);
int tsamd_smooth_run(double *state_a_dev, double *state_b_dev, int32_t stride, const tsamd_smooth_mesh *mesh, const uint8_t *class_dev, int32_t mode, double lam,
                     double mu, int32_t iterations, const float *v0_dev, double max_move, int32_t *result_in_b_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSSPLAT_AMD_H */
