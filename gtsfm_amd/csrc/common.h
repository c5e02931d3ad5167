// Shared helpers for the gfx950 kernels of the GTSfM deep front-end (SuperPoint / SuperGlue / LightGlue).
// CDNA4 only: 64-wide wavefronts, fp32-input MFMA (v_mfma_f32_32x32x2_f32), 160 KiB LDS per CU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define GTSFM_OK 0
#define GTSFM_ERR_INVALID -1
#define GTSFM_ERR_HIP -2
#define GTSFM_ERR_WORKSPACE -3

void gtsfm_set_error(const char* fmt, ...);
// Compute units of the current device (hipDeviceProp_t::multiProcessorCount, read once per process; 256 on an MI355X and the
// fallback when the query fails, e.g. in a build container without a GPU). Launch-geometry thresholds scale with it.
int gtsfm_cu_count(void);

#define GTSFM_CHECK_ARG(cond, ...)        \
    do {                                  \
        if (!(cond)) {                    \
            gtsfm_set_error(__VA_ARGS__); \
            return GTSFM_ERR_INVALID;     \
        }                                 \
    } while (0)

#define GTSFM_CHECK_LAUNCH(name)                                                              \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess) {                                                               \
            gtsfm_set_error("kernel launch failed (%s): %s", name, hipGetErrorString(e_));    \
            return GTSFM_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline size_t a64(size_t floats) { return align_up(floats, 64); }  // pieces of a packed weight blob start at multiples of 64 floats

// Lays a workspace out: consecutive pieces, each starting at a multiple of 256 bytes from `base`. A size query passes a null base and
// reads `used`; a layout that keeps offsets takes them with offset().
struct WorkspaceCarver {
    void* base;
    size_t used;
    size_t offset(size_t bytes) {
        const size_t at = used;
        used += align_up(bytes, 256);
        return at;
    }
    void* take(size_t bytes) { return (void*)((uintptr_t)base + offset(bytes)); }
};

// The two checks every call makes of its workspace: GTSFM_OK, or the status with the error set. `holds` is the caller's verdict, bytes >=
// needed unless it knows of another reason; `sizes` and its arguments say what the bytes are needed for.
__attribute__((format(printf, 6, 7))) static inline int gtsfm_check_workspace(const char* me, const void* base, bool holds, size_t bytes, size_t needed, const char* sizes,
                                                                              ...) {
    GTSFM_CHECK_ARG(base && ((uintptr_t)base & 255) == 0, "%s: the workspace must be aligned to 256 bytes", me);
    if (holds) return GTSFM_OK;
    char what[192];
    va_list args;
    va_start(args, sizes);
    vsnprintf(what, sizeof(what), sizes, args);
    va_end(args);
    gtsfm_set_error("%s: workspace of %zu bytes, %zu needed for %s", me, bytes, needed, what);
    return GTSFM_ERR_WORKSPACE;
}

// Wave-wide reductions over all 64 lanes (result valid in every lane).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
