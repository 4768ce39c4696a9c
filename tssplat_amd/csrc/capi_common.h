// Shared by the translation units that implement the C ABI (capi.cpp and every *_capi.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/tssplat_amd.h"

namespace tsamd {

// Records `msg` as the calling thread's tsamd_last_error() text and returns `code`.
int capi_fail(int code, const std::string &msg);

// Makes `dev` current for the scope of a C-ABI call and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1;
    bool active = false;
    hipError_t enter(int dev)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) return e;
        if (prev != dev) {
            e = hipSetDevice(dev);
            if (e != hipSuccess) return e;
            active = true;
        }
        return hipSuccess;
    }
    ~DeviceGuard()
    {
        if (active) (void)hipSetDevice(prev);
    }
};

// The first null pointer of a list of (pointer, name as in the header) pairs, named on its own: "<name> is null".
struct NamedPtr {
    const void *ptr;
    const char *name;
};
inline int check_not_null(std::initializer_list<NamedPtr> args)
{
    for (const NamedPtr &a : args)
        if (!a.ptr) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string(a.name) + " is null");
    return TSAMD_OK;
}

// ---- the surface stages' argument checks (init_capi.cpp, merge_capi.cpp, metrics_capi.cpp, simplify_capi.cpp, voxel_capi.cpp) ----
inline int check_aligned(const void *ptr, const char *name, uintptr_t bytes)
{
    if (reinterpret_cast<uintptr_t>(ptr) % bytes != 0)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string(name) + " must be " + std::to_string(bytes) + "-byte aligned");
    return TSAMD_OK;
}

// A list of (pointer, name as in the header, alignment in bytes; 1 for bytes): the first null of the list, then the first misaligned one.
struct Buffer {
    const void *ptr;
    const char *name;
    uintptr_t align;
};
inline int check_buffers(std::initializer_list<Buffer> args)
{
    for (const Buffer &a : args)
        if (!a.ptr) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string(a.name) + " is null");
    for (const Buffer &a : args)
        if (int rc = check_aligned(a.ptr, a.name, a.align)) return rc;
    return TSAMD_OK;
}

// "<word> out of range (<least> .. <most>)": nodes or cells per axis
inline int check_grid(int32_t n, int32_t least, int32_t most, const char *word = "grid")
{
    if (n < least || n > most)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string(word) + " out of range (" + std::to_string(least) + " .. " + std::to_string(most) + ")");
    return TSAMD_OK;
}

// The cube [lo, hi]^3 (lo < hi with a finite difference implies that both are finite) ...
inline int check_cube(double lo, double hi)
{
    if (!(lo < hi) || !std::isfinite(hi - lo)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "lo must be below hi, both finite");
    return TSAMD_OK;
}

// ... and where the spacing (hi - lo) / n must not underflow either; `word` is what n counts ("grid", "cells")
inline int check_cube(double lo, double hi, int32_t n, const char *word)
{
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo) && (hi - lo) / double(n) > 0.0))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string("lo / hi must be finite with lo < hi and (hi - lo) / ") + word + " > 0");
    return TSAMD_OK;
}

inline int check_level(float level)
{
    if (std::isnan(level)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "level is NaN");
    return TSAMD_OK;
}

// `what` ("faces", "elem") indexes the vertices with 32 bits
inline int check_vertex_count(int64_t n_vertices, const char *what)
{
    if (n_vertices < 0 || n_vertices > INT32_MAX)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string("n_vertices out of range (0 .. 2^31 - 1: ") + what + " holds 32-bit indices)");
    return TSAMD_OK;
}

// ---- the renderer's argument checks (raster_capi.cpp, shade_capi.cpp) ----
constexpr int64_t kMaxPixels = int64_t(1) << 30;   // pixel and pair-slot (2 per pixel) indices are 32-bit

// cap_pixels: the entry points that index pixels and pair slots with 32 bits (the blend plan and everything under it)
inline int check_image(int64_t batch, int32_t height, int32_t width, bool cap_pixels)
{
    // 8192: snapped window coordinates are kept within +-2^22 sub-pixel units (1/256 pixel) = +-16384 pixels and a triangle with a
    // vertex beyond that is dropped (there is no clipping), so the cap leaves a guard band of at least one screen on every side
    if (batch < 0 || height < 0 || width < 0 || height > 8192 || width > 8192)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "batch / height / width out of range (0 .. 8192 pixels per side)");
    if (cap_pixels && (batch > kMaxPixels || batch * int64_t(height) * width >= kMaxPixels))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "batch x height x width must stay below 2^30 pixels (32-bit pixel and pair indices)");
    return TSAMD_OK;
}

// grid_limit: the entry points that bin triangles (one workgroup per 8 views x 256 triangles)
inline int check_mesh_sizes(int64_t n_vertices, int64_t n_triangles, int64_t batch, bool grid_limit)
{
    if (n_vertices < 0 || n_triangles < 0 || n_triangles > (int64_t(1) << 24) - 1)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "negative size or more than 2^24 - 1 triangles (the id + 1 is returned as a float32, exact up to 2^24)");
    if (grid_limit && (batch + 7) / 8 * 8 * ((n_triangles + 255) / 256) > int64_t(INT32_MAX))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "batch x triangles / 256 exceeds the grid limit (2^31 - 1 workgroups)");
    return TSAMD_OK;
}

}  // namespace tsamd

#define TSAMD_HIP(call)                                                                                         \
    do {                                                                                                        \
        hipError_t e__ = (call);                                                                                \
        if (e__ != hipSuccess)                                                                                  \
            return tsamd::capi_fail(TSAMD_ERR_HIP, std::string(#call) + " failed: " + hipGetErrorString(e__)); \
    } while (0)
