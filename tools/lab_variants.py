#!/usr/bin/env python3
"""Laboratory builds of the tile kernel WITHOUT touching the product source: every variant is a list of textual patches applied
to a COPY of tssplat_amd/csrc/tile_kernel.hip (and, where a patch names it, any other file of _build.SOURCES: the step kernels, the launch
layer, capi.cpp), compiled into tssplat_amd/libtssplat_amd_<name>.so next to
the product library and selected per process with TSSPLAT_AMD_LIB (tools/ab_variants.py does that).  The shipped kernels carry no
experiment switches; pricing builds ("what does this phase cost?": results WRONG on purpose) and candidate
changes live here, reproducible from this file.

    python tools/lab_variants.py --list
    python tools/lab_variants.py nogather nostore ...      # build
    python tools/ab_variants.py base nogather nostore --spheres 512
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tssplat_amd import _build  # noqa: E402

K = "tile_kernel.hip"        # the tile kernel and its dispatch table
S = "step_kernels.hip"       # finish kernel, energy reduction, optimiser kernels
L = "eval_launch.cpp"        # launch recipe, configure_kernels, graphs

# name -> (description, [(file, old, new), ...])
VARIANTS = {
    # ---- pricing builds: one stage removed, results wrong, cost right ----
    "exit_p1": ("leave after pass 1 (stream + F): what the memory phase costs", [
        (K, "    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----",
            "    if (e_b == 12345.678f) g_partials[0] = e_b;\n    if (WITH_GRAD) return;\n    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----")]),
    "noscatter": ("no scatter of the corner forces (table reads and address arithmetic stay)", [
        (K, "                if (p * nq + tid < td.n_slots) {   // (padding slots", "                if (p * nq + tid < td.n_slots && D[p][0] == 12345.678f) {   // (padding slots")]),
    "nogather": ("per-vertex sums skipped (stores of zeros stay)", [
        (K, "            for (int r = 0; r < rows; r += 4) {\n                const LDS_AS float *f[4];", "            for (int r = 0; r < rows && gscale == 12345.678f; r += 4) {\n                const LDS_AS float *f[4];")]),
    "nostore": ("result stores skipped", [
        (K, "            if (v < td.n_verts) {\n                const bool excl = row >= 0;", "            if (v < td.n_verts && gx == 12345.678f) {\n                const bool excl = row >= 0;")]),
    "notail": ("no scatter, no sums, no stores: everything behind pass 3", [
        (K, "                if (p * nq + tid < td.n_slots) {   // (padding slots", "                if (p * nq + tid < td.n_slots && D[p][0] == 12345.678f) {   // (padding slots"),
        (K, "            for (int r = 0; r < rows; r += 4) {\n                const LDS_AS float *f[4];", "            for (int r = 0; r < rows && gscale == 12345.678f; r += 4) {\n                const LDS_AS float *f[4];"),
        (K, "            if (v < td.n_verts) {\n                const bool excl = row >= 0;", "            if (v < td.n_verts && gx == 12345.678f) {\n                const bool excl = row >= 0;")]),
    "nopen3": ("pricing: the inverted-tet branch of pass 3 (F rebuilt, cofactor) skipped -- what moving it out of stage B could buy at most", [
        (K, "                if (scal[p] != 0.f) {  // inverted owned tet: rebuild F", "                if (scal[p] == 12345.678f) {  // inverted owned tet: rebuild F")]),
    # ---- round 6: what could ANY design that hides the stream reach?  (profiles/r06_experiments.md) ----
    "nostream": ("pricing: every tile reads tile 0's planes (L2 hits: the stream costs almost nothing, results wrong) at the production occupancy -- "
                 "the floor of a PERFECT next-tile prefetch with two workgroups per CU", [
        (K, "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + td.blob_off);", "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + (td.blob_off & 0));")]),
    "nostream32": ("pricing: tile t reads the planes of tile t mod 32 (2.6 MB: L2 / MALL hits spread over all channels -- `nostream` "
                   "hammers ONE tile's 80 KB from every CU and is slower than the real stream) at the production occupancy", [
        (K, "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + td.blob_off);", "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + a.tiles[tile & 31].blob_off);")]),
    "onewg_nostream32": ("pricing: one workgroup per CU AND the planes from L2 (tile t mod 32) -- the floor of the LDS-DMA loader / consumer design", [
        (K, "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + td.blob_off);", "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + a.tiles[tile & 31].blob_off);"),
        (L, "        r.tile_lds = size_t(e.lds_bytes);", "        r.tile_lds = size_t(100 * 1024);"),
        (L, "    if (lds_bytes <= configured[dev]) return hipSuccess;", "    lds_bytes = 100 * 1024;\n    if (lds_bytes <= configured[dev]) return hipSuccess;")]),
    "onewg_exit_p1": ("pricing: one workgroup per CU, leave after pass 1 -- stage A of a LONE workgroup (stream + F); `onewg` minus this = the chain of passes a "
                      "lone 12-wave workgroup needs behind it, i.e. what a loader / consumer workgroup's consumers would still have to do per tile", [
        (K, "    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----",
            "    if (e_b == 12345.678f) g_partials[0] = e_b;\n    if (WITH_GRAD) return;\n    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----"),
        (L, "        r.tile_lds = size_t(e.lds_bytes);", "        r.tile_lds = size_t(100 * 1024);"),
        (L, "    if (lds_bytes <= configured[dev]) return hipSuccess;", "    lds_bytes = 100 * 1024;\n    if (lds_bytes <= configured[dev]) return hipSuccess;")]),
    "fold_price": ("pricing: NO finish launch; every workgroup ends with a device-scope release fence + one atomic on a counter (in the first dword of the "
                   "energy partials' last pair: results wrong) -- the floor of a finish folded into the tile kernel for small plans (the last tile of a "
                   "sphere to arrive sums its shared vertices, the last of all reduces the energy)", [
        (K, "        if (64 * nw < td.n_verts) {   // more vertices than lanes (rare;", 
            "        __threadfence();\n        __syncthreads();\n        if (tid == 0) atomicAdd(reinterpret_cast<unsigned int *>(a.partials + 2 * size_t(a.n_tiles)), 1u);\n        if (64 * nw < td.n_verts) {   // more vertices than lanes (rare;"),
        (L, "    if (f.n_finish > 0) {\n        r.finish_fn = step_kernels().finish;", "    if (f.n_finish < 0) {\n        r.finish_fn = step_kernels().finish;"),
        (L, "    } else if (f.energy) {\n        r.finish_fn = step_kernels().energy_reduce;", "    } else if (f.energy && !e.grad) {\n        r.finish_fn = step_kernels().energy_reduce;"),
        ("capi.cpp", "upload(h->d_partials, nullptr, P.tiles.size() * 2, h->device_bytes)", "upload(h->d_partials, nullptr, P.tiles.size() * 2 + 2, h->device_bytes)")]),
    "ntstore_excl": ("candidate: non-temporal stores for the EXCLUSIVE result rows (grad: not read again by this evaluation); staging rows stay temporal", [
        (K, "                dst[0] = gx * sc;\n                dst[1] = gy * sc;\n                dst[2] = gz * sc;",
            "                if (excl) {\n                    __builtin_nontemporal_store(gx * sc, dst);\n                    __builtin_nontemporal_store(gy * sc, dst + 1);\n                    __builtin_nontemporal_store(gz * sc, dst + 2);\n                } else {\n                    dst[0] = gx * sc;\n                    dst[1] = gy * sc;\n                    dst[2] = gz * sc;\n                }")]),
    "fin_nodep": ("pricing: the finish kernel's staging rows at an address computed from the vertex number (2 or 3 rows from 2.5 k: results wrong) instead of "
                  "from fin_off[k] -- what a class-major staging layout (rows at computable addresses, one dependent level less) could buy at most", [
        (S, "        const int32_t e0 = FIN_LOAD(&a.fin_off[k]), e1 = FIN_LOAD(&a.fin_off[k + 1]);   // consecutive rows, tile order",
            "        const int32_t e0 = int32_t((k * 5) >> 1), e1 = e0 + 2 + int32_t(k & 1);   // (pricing)")]),
    "ntfinish": ("the finish kernel's loads non-temporal (measured: finish kernel +50 %)", [(S, "#define FIN_LOAD(p) (*(p))", "#define FIN_LOAD(p) __builtin_nontemporal_load(p)")]),
    "onewg": ("pricing: ONE workgroup per CU (100 KiB of dynamic LDS requested per workgroup, same tiles, same kernel)", [
        (L, "        r.tile_lds = size_t(e.lds_bytes);", "        r.tile_lds = size_t(100 * 1024);"),
        (L, "    if (lds_bytes <= configured[dev]) return hipSuccess;", "    lds_bytes = 100 * 1024;\n    if (lds_bytes <= configured[dev]) return hipSuccess;")]),
    "onewg_nostream": ("pricing: one workgroup per CU AND no stream -- the floor of the LDS-DMA loader / consumer design (a CU's LDS holds ONE tile's records "
                       "next to the next tile's ring; 1 024 threads per workgroup cap the consumers at 12 waves + 4 loaders)", [
        (K, "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + td.blob_off);", "reinterpret_cast<const GLOBAL_AS uint32_t *>(g_blob + (td.blob_off & 0));"),
        (L, "        r.tile_lds = size_t(e.lds_bytes);", "        r.tile_lds = size_t(100 * 1024);"),
        (L, "    if (lds_bytes <= configured[dev]) return hipSuccess;", "    lds_bytes = 100 * 1024;\n    if (lds_bytes <= configured[dev]) return hipSuccess;")]),
    "rows8": ("candidate: per-vertex sums walk EIGHT rows per trip instead of four (a.veg's fullest vertices carry up to 56 rows: 7 dependent LDS round trips instead of 14)", [
        (K, "            for (int r = 0; r < rows; r += 4) {\n                const LDS_AS float *f[4];\n#pragma unroll\n                for (int u = 0; u < 4; ++u) {",
            "            for (int r = 0; r < rows; r += 8) {\n                const LDS_AS float *f[8];\n#pragma unroll\n                for (int u = 0; u < 8; ++u) {"),
        (K, "#pragma unroll\n                for (int u = 0; u < 4; ++u) {\n                    gx += f[u][0];",
            "#pragma unroll\n                for (int u = 0; u < 8; ++u) {\n                    gx += f[u][0];")]),
    # ---- candidates ----
    "stagger": ("the second workgroup of every CU starts half a tile late (first 512 workgroups: 256-511 sleep ~2.7 us)", [
        (K, "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n",
            "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n    if (blockIdx.x >= 256 && blockIdx.x < 512)\n        __builtin_amdgcn_s_sleep(100);   // (64 clocks per unit: 6 400 clocks)\n")]),
    "staggerL": ("the workgroup whose LDS allocation does not start at 0 (= the second one of its CU) starts 6 400 clocks late, first 512 workgroups only", [
        (K, "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n",
            "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n    if (blockIdx.x < 512 && (__builtin_amdgcn_s_getreg((11 << 11) | 6) & 0xfff) != 0) __builtin_amdgcn_s_sleep(100);\n")]),
    "staggerL2": ("same, 3 840 clocks", [
        (K, "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n",
            "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n    if (blockIdx.x < 512 && (__builtin_amdgcn_s_getreg((11 << 11) | 6) & 0xfff) != 0) __builtin_amdgcn_s_sleep(60);\n")]),
    "staggerJ": ("odd workgroups of an XCD among its first 64 start 6 400 clocks late", [
        (K, "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n",
            "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n    if (jb < 64 && (jb & 1)) __builtin_amdgcn_s_sleep(100);\n")]),
    "stagger2": ("same, ~1.3 us", [
        (K, "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n",
            "    if (jb >= a.tiles_per_xcd || tile >= tile_end) return;\n    if (blockIdx.x >= 256 && blockIdx.x < 512)\n        __builtin_amdgcn_s_sleep(50);\n")]),
    "nofence": ("no scheduling fence between a lane's slots", [
        (K, "#define SLOT_FENCE() __builtin_amdgcn_sched_barrier(0)", "#define SLOT_FENCE() ((void)0)")]),
    "nokeeph": ("own H re-read from LDS in pass 3 (18 VGPRs less across the barrier)", [
        (K, "constexpr int kKeepF = SPT, kKeepH = WEIGHTED ? 0 : SPT;", "constexpr int kKeepF = SPT, kKeepH = 0;")]),
    "keepf3": ("own F kept in registers through pass 3 (own H re-read from LDS): an inverted tet's F is not rebuilt", [
        (K, "constexpr int kKeepF = SPT, kKeepH = WEIGHTED ? 0 : SPT;", "constexpr int kKeepF = SPT, kKeepH = 0;"),
        (K, "                    const uint32_t w0 = q_lv01[p], w1 = q_lv23[p];\n                    float F[9], C[9];\n                    slot_F(kXS, pos_lo(w0), pos_hi(w0), pos_lo(w1), pos_hi(w1), dm, p, F);\n                    cof3(F, C);",
            "                    float C[9];\n                    cof3(Fk[p], C);")]),
    "b96": ("12-byte LDS accesses of the force array as ONE instruction each (ds_write_b96 / ds_read_b96)", [
        (K, "                    f0[0] = (-d[0] - d[3]) - d[6], f0[1] = (-d[1] - d[4]) - d[7], f0[2] = (-d[2] - d[5]) - d[8];   // (= -(f1 + f2 + f3), bit for bit)\n                    f1[0] = d[0], f1[1] = d[1], f1[2] = d[2];\n                    f2[0] = d[3], f2[1] = d[4], f2[2] = d[5];\n                    f3[0] = d[6], f3[1] = d[7], f3[2] = d[8];",
            "                    typedef float v3f __attribute__((ext_vector_type(3)));\n                    const v3f q0 = {-(d[0] + d[3] + d[6]), -(d[1] + d[4] + d[7]), -(d[2] + d[5] + d[8])}, q1 = {d[0], d[1], d[2]}, q2 = {d[3], d[4], d[5]}, q3 = {d[6], d[7], d[8]};\n                    asm volatile(\"ds_write_b96 %0, %1\" : : \"v\"(fdst[p][0]), \"v\"(q0) : \"memory\");\n                    asm volatile(\"ds_write_b96 %0, %1\" : : \"v\"(fdst[p][1]), \"v\"(q1) : \"memory\");\n                    asm volatile(\"ds_write_b96 %0, %1\" : : \"v\"(fdst[p][2]), \"v\"(q2) : \"memory\");\n                    asm volatile(\"ds_write_b96 %0, %1\" : : \"v\"(fdst[p][3]), \"v\"(q3) : \"memory\");\n                    (void)f0; (void)f1; (void)f2; (void)f3;")]),
    "fma4": ("4 * own - first neighbour as one fused multiply-add per entry (5 instructions less per gathered slot and pass)", [
        (K, """    Mat9 g0 = load_slot(nb[0]);
    acc.p01 *= 4.f; acc.p23 *= 4.f; acc.p45 *= 4.f; acc.p67 *= 4.f;
    acc.p8 *= 4.f;
    Mat9 g1 = load_slot(nb[1]);
    sub9(acc, g0);""", """    Mat9 g0 = load_slot(nb[0]);
    Mat9 g1 = load_slot(nb[1]);
    const v2f four = {4.f, 4.f};
    acc.p01 = __builtin_elementwise_fma(acc.p01, four, -g0.p01); acc.p23 = __builtin_elementwise_fma(acc.p23, four, -g0.p23);
    acc.p45 = __builtin_elementwise_fma(acc.p45, four, -g0.p45); acc.p67 = __builtin_elementwise_fma(acc.p67, four, -g0.p67);
    acc.p8 = __builtin_fmaf(acc.p8, 4.f, -g0.p8);""")]),
    "sdwa": ("row-table address of a corner in one SDWA instruction ((w >> 8) & 0xfc = byte 1 of the field & 0xfc)", [
        (K, """            const uint32_t r0 = *lds_at<const uint32_t>((w0 >> 8) & 0xfcu), r1 = *lds_at<const uint32_t>((w0 >> 24) & 0xfcu),
                           r2 = *lds_at<const uint32_t>((w1 >> 8) & 0xfcu), r3 = *lds_at<const uint32_t>((w1 >> 24) & 0xfcu);""",
            """            uint32_t ta0, ta1, ta2, ta3;
            const uint32_t kfc = 0xfcu;
            asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(ta0) : "s"(kfc), "v"(w0));
            asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(ta1) : "s"(kfc), "v"(w0));
            asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(ta2) : "s"(kfc), "v"(w1));
            asm("v_and_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(ta3) : "s"(kfc), "v"(w1));
            const uint32_t r0 = *lds_at<const uint32_t>(ta0), r1 = *lds_at<const uint32_t>(ta1), r2 = *lds_at<const uint32_t>(ta2), r3 = *lds_at<const uint32_t>(ta3);""")]),
    "fs": ("fma4 + sdwa", []),
    "prioA": ("wave priority by stage: pass 1 = 0, pass 2 = 1, pass 3 = 2, tail = 3", [
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(1);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(2);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
    ]),
    "prioB": ("head (load issue) = 3, pass 1 = 0, pass 2 = 1, pass 3 = 2, tail = 3", [
        (K, '    const int32_t gv0 = INDEX_NT ? __builtin_nontemporal_load(gv_ptr) : *gv_ptr;\n', '    const int32_t gv0 = INDEX_NT ? __builtin_nontemporal_load(gv_ptr) : *gv_ptr;\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(1);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(2);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
    ]),
    "prioC": ("pass 1 = 0, everything behind it = 3", [
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
    ]),
    "prioD": ("reversed: pass 1 = 3, pass 2 = 2, pass 3 = 1, tail = 0", [
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(2);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(1);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
    ]),
    "prioE": ("head = 3, pass 1 = 1, pass 2 = 2, pass 3 = 3, tail = 3", [
        (K, '    const int32_t gv0 = INDEX_NT ? __builtin_nontemporal_load(gv_ptr) : *gv_ptr;\n', '    const int32_t gv0 = INDEX_NT ? __builtin_nontemporal_load(gv_ptr) : *gv_ptr;\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(1);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(2);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
    ]),
    "prioF": ("pass 1 = 0, pass 2 = 0, pass 3 = 2, tail = 3", [
        (K, '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n', '    // ---- pass 1: F = Ds Dm^-1, inversion penalty ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
        (K, '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n', '    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----\n' + "    " + '__builtin_amdgcn_s_setprio(0);\n'),
        (K, '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n', '        // ---- pass 3: P = L^T H + (c2 / c1) dpen cof(F);  d = P Dm^-T (per-tet vertex forces, c1 applied at the end) ----\n' + "    " + '__builtin_amdgcn_s_setprio(2);\n'),
        (K, '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n', '        // ---- scatter the vertex forces: (f0, f1, f2, f3), f0 = -(f1 + f2 + f3), 12 bytes each ----\n' + "    " + '__builtin_amdgcn_s_setprio(3);\n'),
    ]),
    "identblocks": ("vertex blocks of the per-vertex sums in wave order (no reversal of waves 4-7)", [
        (K, "        if (wave & 4) {   // (a permutation", "        if (false) {   // (a permutation")]),
}


_T = "__builtin_amdgcn_s_memrealtime()"   # 100 MHz timestamp
# the product kernel's phases as seen by wave 0 of a few mid-launch workgroups (two workgroups per CU: each one's phases stretch by what the other takes)
_BLK = "(blockIdx.x == 4000 || blockIdx.x == 4003 || blockIdx.x == 7001 || blockIdx.x == 9002 || blockIdx.x == 12005 || blockIdx.x == 15000)"
VARIANTS["stamps"] = ("product kernel + 100 MHz phase timestamps of wave 0 in six mid-launch workgroups (printf; run a handful of evaluations only)", [(_f, _o, _n.replace("@T@", _T).replace("@BLK@", _BLK)) for _f, _o, _n in [
    (K, "    const TileDesc td = a.tiles[tile];", "    unsigned long long ts[8];\n    ts[0] = @T@;\n    const TileDesc td = a.tiles[tile];"),
    (K, "    __syncthreads();\n    // behind the barrier: what pass 2 and the end of the tile need", "    __syncthreads();\n    ts[1] = @T@;\n    // behind the barrier: what pass 2 and the end of the tile need"),
    (K, "    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----", "    ts[2] = @T@;\n    // ---- pass 2: H = L F on owned slots (0 on halo slots), E_s = 1/2 |H|^2 ----"),
    (K, "    __syncthreads();  // every read of F is done; overwrite it with H in place", "    __syncthreads();  // every read of F is done; overwrite it with H in place\n    ts[3] = @T@;"),
    (K, "        publish_wave_sums();\n        __syncthreads();   // (the wave pairs are in red[]; sum_waves() at the end of the tile)\n",
        "        publish_wave_sums();\n        __syncthreads();   // (the wave pairs are in red[]; sum_waves() at the end of the tile)\n        ts[4] = @T@;\n"),
    (K, "        __syncthreads();   // all waves done with H and with the staged positions", "        __syncthreads();   // all waves done with H and with the staged positions\n        ts[5] = @T@;"),
    (K, "        __syncthreads();\n\n        // ---- per-vertex sums: lane = vertex", "        __syncthreads();\n        ts[6] = @T@;\n\n        // ---- per-vertex sums: lane = vertex"),
    (K, "    }\n#undef t_own\n", """        ts[7] = @T@;
        if ((tid == 0 || tid == 704) && @BLK@)
            printf("blk %d wave %d (x10 ns): positions %llu pass1 %llu pass2 %llu H-stored %llu pass3 %llu scatter %llu sums+stores %llu | total %llu\\n", int(blockIdx.x), tid >> 6,
                   ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2], ts[4] - ts[3], ts[5] - ts[4], ts[6] - ts[5], ts[7] - ts[6], ts[7] - ts[0]);
    }
#undef t_own
""")]])

# ... and the inside of the per-vertex sums (wave 0 = the block of the fullest vertices): row loop / wait for the destination ids / stores issued
VARIANTS["stamps2"] = ("stamps + the per-vertex sums split into row loop, wait for vdst, stores", [(_f, _o, _n.replace("@T@", _T).replace("@BLK@", _BLK)) for _f, _o, _n in [
    (K, "    const TileDesc td = a.tiles[tile];", "    unsigned long long ts[4];\n    int sum_rows = 0;\n    const TileDesc td = a.tiles[tile];"),
    (K, "        __syncthreads();\n\n        // ---- per-vertex sums: lane = vertex", "        __syncthreads();\n        ts[0] = @T@;\n\n        // ---- per-vertex sums: lane = vertex"),
    (K, "            if (v < td.n_verts) {\n                const bool excl = row >= 0;", "            sum_rows = rows;\n            asm volatile(\"\" : \"+v\"(gx), \"+v\"(gy), \"+v\"(gz));\n            ts[1] = @T@;\n            asm volatile(\"\" : \"+v\"(row));\n            asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n            ts[2] = @T@;\n            if (v < td.n_verts) {\n                const bool excl = row >= 0;"),
    (K, "    }\n#undef t_own\n", """        ts[3] = @T@;
        if ((tid == 0 || tid == 64 || tid == 192) && @BLK@)
            printf("blk %d wave %d (x10 ns): rows %d: row loop %llu, wait for vdst %llu, stores issued %llu\\n", int(blockIdx.x), tid >> 6, sum_rows, ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2]);
    }
#undef t_own
""")]])

# Is the acknowledgement of the energy-partial store on the workgroup's critical path?  Wave 0 and the LAST wave (the one that adds up the wave
# pairs and stores the tile's (E_s, E_b)) of the same six workgroups, all times from the H-store barrier on: `drained` = an explicit
# s_waitcnt vmcnt(0) where the compiler's own stands at the head of pass 3 (behind the store in `ack_stamps_early`: the store's acknowledgement),
# `pass3 done` = the wave arrives at the pre-scatter barrier, `barrier left` = the workgroup's last wave has arrived, then scatter, sums + stores
# (wave 0: the row walk, whose first trip holds the compiler's other vmcnt(0), for dst_row) and `partials acked` = the reduction at the end of the tile
# and the acknowledgement of its store.  t0 (the low digits of the 100 MHz clock at the H-store barrier) puts the two waves of a workgroup on one axis.
_ACK = [(_f, _o, _n.replace("@T@", _T).replace("@BLK@", _BLK)) for _f, _o, _n in [
    (K, "    const TileDesc td = a.tiles[tile];", "    unsigned long long ts[7];\n    const TileDesc td = a.tiles[tile];"),
    (K, "        __syncthreads();   // (the wave pairs are in red[]; sum_waves() at the end of the tile)\n",
        "        __syncthreads();   // (the wave pairs are in red[]; sum_waves() at the end of the tile)\n        ts[0] = @T@;\n        //@EARLY@\n"
        "        asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\");\n        ts[1] = @T@;\n"),
    (K, "        __syncthreads();   // all waves done with H and with the staged positions", "        ts[2] = @T@;\n        __syncthreads();   // all waves done with H and with the staged positions\n        ts[3] = @T@;"),
    (K, "        __syncthreads();\n\n        // ---- per-vertex sums: lane = vertex", "        __syncthreads();\n        ts[4] = @T@;\n\n        // ---- per-vertex sums: lane = vertex"),
    (K, "        sum_waves();   // the tile's (E_s, E_b): the last wave's last instruction, its acknowledgement behind wave 0's row walk\n    }\n", """        ts[5] = @T@;
        //@LATE@
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ts[6] = @T@;
        if ((tid == 0 || (nw > 1 && tid == 64 * (nw - 1))) && @BLK@)
            printf("blk %d wave %d of %d (x10 ns from the H-store barrier, t0 %llu): drained %llu pass3 done %llu barrier left %llu scatter done %llu sums+stores done %llu partials acked %llu\\n",
                   int(blockIdx.x), wave, nw, ts[0] % 100000ull, ts[1] - ts[0], ts[2] - ts[0], ts[3] - ts[0], ts[4] - ts[0], ts[5] - ts[0], ts[6] - ts[0]);
    }
""")]]
VARIANTS["ack_stamps"] = ("product kernel + stamps of wave 0 and the last wave around pass 3 and the end of the tile (printf; run a handful of evaluations only)",
                          [(_f, _o, _n.replace("//@LATE@", "sum_waves();").replace("        //@EARLY@\n", "")) for _f, _o, _n in _ACK])
VARIANTS["ack_stamps_early"] = ("ack_stamps with the reduction where it stood before: right behind the H-store barrier, its store in front of pass 3",
                                [(_f, _o, _n.replace("//@EARLY@", "sum_waves();").replace("        //@LATE@\n", "")) for _f, _o, _n in _ACK])

# candidate (round 6, from the stamps): the row loop of the per-vertex sums is one wave's dependent chain -- ~45 instructions per four rows, then a
# wait for eight LDS reads: 0.17 us per trip, 2.3 us for a.veg's 56-row hubs (wave 0 is the last wave of its workgroup by that much).  Two trips in
# flight: the reads of trip k + 1 are issued before trip k is added up (same order of additions: bit-identical results).
VARIANTS["sums_pipe"] = ("candidate: per-vertex sums software-pipelined, two trips of four rows in flight", [
    (K, """            for (int r = 0; r < rows; r += 4) {
                const LDS_AS float *f[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t base = uint32_t(__builtin_amdgcn_readlane(int(tab), r + u)), w = uint32_t(__builtin_amdgcn_readlane(int(wid), r + u));
                    f[u] = lds_at<const float>(v12 < w ? base + v12 : kZeroEntry);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    gx += f[u][0];
                    gy += f[u][1];
                    gz += f[u][2];
                }
            }""", """            float A[4][3], B[4][3];
            auto fetch = [&](int r, float (&d)[4][3]) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t base = uint32_t(__builtin_amdgcn_readlane(int(tab), r + u)), w = uint32_t(__builtin_amdgcn_readlane(int(wid), r + u));
                    const LDS_AS float *f = lds_at<const float>(v12 < w ? base + v12 : kZeroEntry);
                    d[u][0] = f[0], d[u][1] = f[1], d[u][2] = f[2];
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            auto add = [&](const float (&d)[4][3]) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    gx += d[u][0];
                    gy += d[u][1];
                    gz += d[u][2];
                }
                __builtin_amdgcn_sched_barrier(0);
            };
            if (rows > 0) {
                fetch(0, A);
                int r = 4;
                for (; r + 4 < rows; r += 8) {   // trips r / 4 and r / 4 + 1 both exist
                    fetch(r, B);
                    add(A);
                    fetch(r + 4, A);
                    add(B);
                }
                if (r < rows) {
                    fetch(r, B);
                    add(A);
                    add(B);
                } else {
                    add(A);
                }
            }""")])

# ---- the nearest-point search of the surface metrics (tools/bench_metrics.py --variants prices them; all give the product's bits) ----
M = "metrics_kernels.hip"
for _q in (2, 8):
    VARIANTS[f"nearest_q{_q}"] = (f"nearest points: {_q} queries per lane instead of 4 (the automatic chunk rule still counts blocks of 4: pass ref_chunks)",
                                  [(M, "constexpr int kQ = kNearestQueriesPerLane;", f"constexpr int kQ = {_q};")])
for _t in (256, 4096):
    VARIANTS[f"nearest_tile{_t}"] = (f"nearest points: ref tiles of {_t} points instead of 1024", [(M, "constexpr int kTile = kNearestTile;", f"constexpr int kTile = {_t};")])
VARIANTS["nearest_selects"] = ("nearest points: a compare and two selects per pair (11.3 VALU per pair) instead of the minimum of each group of 8 ref points and "
                               "the rare scan for its index -- the loop the kernel started with (profiles/metrics_bench.json)", [
    (M, """float4 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = tile[j + u];
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                uint32_t bits[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float dx = qx[k] - r[u].x, dy = qy[k] - r[u].y, dz = qz[k] - r[u].z;
                    bits[u] = __float_as_uint((dx * dx + dy * dy) + dz * dz);
                }
                const uint32_t m = min(min(min(bits[0], bits[1]), min(bits[2], bits[3])), min(min(bits[4], bits[5]), min(bits[6], bits[7])));
                if (m < best[k]) {                             // rare once the stream is a few thousand points old
                    best[k] = m;
                    int32_t at = 7;
#pragma unroll
                    for (int u = 6; u >= 0; --u) at = bits[u] == m ? u : at;
                    arg[k] = int32_t(base) + j + at;           // the lowest index of the group's minimum
                }
            }""", """#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 r = tile[j + u];
                const int32_t id = int32_t(base) + j + u;
#pragma unroll
                for (int k = 0; k < kQ; ++k) {
                    const float dx = qx[k] - r.x, dy = qy[k] - r.y, dz = qz[k] - r.z;
                    const uint32_t bits = __float_as_uint((dx * dx + dy * dy) + dz * dz);
                    const bool less = bits < best[k];
                    best[k] = less ? bits : best[k];
                    arg[k] = less ? id : arg[k];
                }
            }""")])

# ---- the exact point-to-triangle search (tools/bench_metrics.py --exact prices them; all but pointmesh_count give the product's bits) ----
PM = "pointmesh_kernels.hip"
for _q in (2, 4):
    VARIANTS[f"pointmesh_q{_q}"] = (f"point to mesh: {_q} queries per lane instead of 1 (the automatic chunk rule still counts blocks of 1: pass ref_chunks)",
                                    [(PM, "constexpr int kQ = kPointMeshQueriesPerLane;", f"constexpr int kQ = {_q};")])
VARIANTS["pointmesh_tile256"] = ("point to mesh: LDS tiles of 256 bounding spheres instead of 1024", [(PM, "constexpr int kTile = kPointMeshTile;", "constexpr int kTile = 256;")])
VARIANTS["pointmesh_noprune"] = ("point to mesh: no bounding-sphere test -- every pair of a query and a valid triangle takes the float64 evaluation (the same bits)", [
    (PM, "    return (dx * dx + dy * dy) + dz * dz <= reach * reach;", "    (void)dx, (void)dy, (void)dz, (void)reach;\n    return s.w == s.w;")])
VARIANTS["pointmesh_count"] = ("point to mesh: tri_out holds the number of float64 evaluations of the query's search (seed and finish not counted) instead of the "
                               "triangle -- the share of pairs that pass the sphere test", [
    (PM, "int64_t per_chunk,\n                                                                           unsigned long long *keys)",
     "int64_t per_chunk,\n                                                                           unsigned long long *keys, unsigned *counts)"),
    (PM, "    unsigned long long best[kQ];\n", "    unsigned long long best[kQ];\n    unsigned evaluated[kQ] = {};\n"),
    (PM, "                        if (key < best[k]) {\n", "                        ++evaluated[k];\n                        if (key < best[k]) {\n"),
    (PM, "        if (q < n && best[k] != kNoKey) atomicMin(keys + q, best[k]);\n",
     "        if (q < n && best[k] != kNoKey) atomicMin(keys + q, best[k]);\n        if (q < n) atomicAdd(counts + q, evaluated[k]);\n"),
    (PM, "                       corners, n_triangles, per_chunk, keys);\n",
     "                       corners, n_triangles, per_chunk, keys, reinterpret_cast<unsigned *>(seed_idx));\n"),
    (PM, "    hipLaunchKernelGGL(pointmesh_seed_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, query, n, corners, n_triangles, seed_idx, keys);\n",
     "    hipLaunchKernelGGL(pointmesh_seed_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, query, n, corners, n_triangles, seed_idx, keys);\n"
     "    if (hipMemsetAsync(seed_idx, 0, size_t(n) * sizeof(int32_t), stream) != hipSuccess) return hipErrorUnknown;   // dead after the seed kernel: the counters\n"),
    (PM, "n_triangles, keys, d2_out, tri_out, point_out);\n    return hipGetLastError();",
     "n_triangles, keys, d2_out, tri_out, point_out);\n"
     "    if (hipMemcpyAsync(tri_out, seed_idx, size_t(n) * sizeof(int32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess) return hipErrorUnknown;\n"
     "    return hipGetLastError();")])

COMBOS = {"fs": ["fma4", "sdwa"], "stamps_rows8": ["stamps", "rows8"]}    # ("undef" -- inactive lanes' arrays left undefined -- was adopted by the product kernel)


FLAG_VARIANTS = {   # compiler-flag builds of the unpatched source: name -> function(list of device flags) -> list
    "sched_default": lambda f: [x for x in f if x not in ("-mllvm", "-amdgpu-sched-strategy=max-ilp")],
    "sched_memclause": lambda f: [("-amdgpu-sched-strategy=max-memory-clause" if x == "-amdgpu-sched-strategy=max-ilp" else x) for x in f],
    "sched_iterilp": lambda f: [("-amdgpu-sched-strategy=iterative-ilp" if x == "-amdgpu-sched-strategy=max-ilp" else x) for x in f],
}
# -D builds: the define goes to EVERY translation unit (host and device), the source is unpatched
DEFINE_VARIANTS = {
    "unpaired": ("the device image of rounds 1-5: planes one after the other, thirteen 8-byte loads per lane (the product interleaves the planes that are "
                 "loaded together: six 16-byte + one 8-byte load, plan.h: planes_paired)", ["-DTSAMD_PAIRED_PLANES=0"]),
}
for _n, (_d, _f) in DEFINE_VARIANTS.items():
    VARIANTS[_n] = (_d, [])
VARIANTS["stamps_rows8"] = ("stamps on top of rows8: does halving the longest walk shorten the workgroup, and what do the other phases do?", [])
for _n in FLAG_VARIANTS:
    VARIANTS[_n] = (f"compiler flags: {_n}", [(K, "// gfx950 (MI355X / CDNA4) kernels", "// gfx950 (MI355X / CDNA4) kernels")])


def patched_sources(name: str) -> dict:
    """file -> patched text of every file the variant touches (a combination: its parts' patches in turn).  Text only, no
    compiler.  LookupError when an anchor is no longer in its file (tests/test_lab_variants.py asks every variant)."""
    patches = [q for n in COMBOS[name] for q in VARIANTS[n][1]] if name in COMBOS else VARIANTS[name][1]
    srcs = {}
    for f, old, new in patches:
        if f not in srcs:
            srcs[f] = open(os.path.join(_build.CSRC, f)).read()
        if old not in srcs[f]:
            raise LookupError(f"variant {name}: patch anchor not found in {f}: {old[:70]!r}")
        srcs[f] = srcs[f].replace(old, new)
    return srcs


def build(name: str) -> str:
    if name in DEFINE_VARIANTS:
        return _build.build_variant(name, DEFINE_VARIANTS[name][1])
    try:
        srcs = patched_sources(name)
    except LookupError as e:
        raise SystemExit(str(e))
    hipcc = _build._hipcc()
    _build.build()                                      # the product objects of everything that is not patched
    os.makedirs(_build._OBJ, exist_ok=True)
    objs = []
    for src in _build.SOURCES:
        obj = os.path.join(_build._OBJ, os.path.splitext(src)[0] + ".o")
        if src in srcs:
            patched = os.path.join(_build.CSRC, f"_lab_{name}_{src}")      # (next to the original: relative includes resolve)
            open(patched, "w").write(srcs[src])
            obj = os.path.join(_build._OBJ, f"{os.path.splitext(src)[0]}_lab_{name}.o")
            try:
                if src.endswith(".hip"):
                    dflags = FLAG_VARIANTS[name](list(_build.DEVICE_FLAGS)) if name in FLAG_VARIANTS else _build.DEVICE_FLAGS
                    cmd = [hipcc, "-c", patched, "-o", obj] + _build.HOST_FLAGS + dflags + _build.SOURCE_FLAGS.get(src, [])
                else:
                    cmd = [hipcc] + _build.HOST_FLAGS + ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-c", patched, "-o", obj]
                subprocess.check_call(cmd)
            finally:
                os.remove(patched)
        objs.append(obj)
    out = os.path.join(os.path.dirname(_build.LIB), f"libtssplat_amd_{name}.so")
    subprocess.check_call([hipcc, "-shared", "-o", out] + objs + [f"--offload-arch={_build.ARCH}", "-pthread"])
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] == "--list":
        for k, (d, _) in VARIANTS.items():
            print(f"{k:14s} {d}")
        raise SystemExit(0)
    for n in sys.argv[1:]:
        print(build(n))
