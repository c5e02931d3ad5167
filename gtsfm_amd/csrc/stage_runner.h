// How a geometry pipeline (the view graph, 1DSfM, triangulation) runs its stages: two runners with one interface, so that a pipeline is ONE
// function template over the runner. The extern "C" call launches it with a DeviceRunner; the stand-alone host programs under tools/ walk
// the same function with a HostRunner on a CPU, under the sanitizers. Bounds, scan order, flag reads and their wording, round loops and
// conditional stages are therefore written once. Internal linkage; compiles in both passes of hipcc.
//
//   each<Tag>(n, f)            f(i) for every i in 0 .. n - 1: one index per lane, launch_grid(n, THREADS) workgroups.
//   group<Tag, T, L>(m, f)     f(group, lane, lanes) for m groups of L lanes, T / L groups per workgroup: a wave per edge, a workgroup per
//                              track, or a capped grid whose lanes stride (first = group * lanes + lane, stride = m * lanes).
//   scan(val, n)               val[0 .. n) -> its exclusive prefix sum in place, val[n] = the total.
//   fetch(dst, src, count, what)  count elements from the device to the host, complete on return: an asynchronous copy and a stream
//                              wait. A failure is worded "<entry point>: <what> failed: <the runtime's reason>".
//   copy(dst, src, count, what)   the copy alone, complete when the fetch that follows it returns: two values cost one wait.
//   zero(p, bytes)
//   block(name, launch, host)  a block-cooperative kernel stays an ordinary kernel: launch(stream) launches it, host(runner) is the plain
//                              loop that stands in for it on a CPU and is written next to it.
// Tag is a type that only names the stage: it is part of the kernel's symbol, so a trace lists vg_edge_degree_stage and not a lambda's
// number. f is a STAGE_FN lambda taken by value.
//
// A runner keeps the first failure -- a launch that the runtime refuses, a copy, a wait, a memset: `status` leaves GTSFM_OK with the error
// worded, every later call does nothing and returns it. A pipeline therefore looks at the status where it needs a value on the host
// (fetch) and when it returns, and must return run.status (or a refusal of its own), never a literal GTSFM_OK.
//
// HostRunner{descending, device_lanes}: {false, false} walks every stage in ascending order with one lane per group; {true, true} walks
// in descending order with the device's lane count, the last lane first. The atomics are plain updates on a CPU (graph_prims.h), so the
// two hand out list slots in opposite orders; a pipeline's outputs must not depend on it.
#pragma once

#include <string.h>

#include "graph_prims.h"

#define STAGE_THREADS 256
#define STAGE_FN [=] __host__ __device__

namespace {

template <int THREADS, int BOUNDS, class Tag, class F>
__global__ __launch_bounds__(BOUNDS) void index_stage_kernel(long long n, F f) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) f(i);
}

template <int THREADS, int LANES, class Tag, class F>
__global__ __launch_bounds__(THREADS) void group_stage_kernel(long long groups, F f) {
    // a group that is the whole workgroup keeps its index uniform (scalar registers), as blockIdx.x alone
    const long long group = LANES == THREADS ? (long long)blockIdx.x : (long long)blockIdx.x * (THREADS / LANES) + threadIdx.x / LANES;
    if (group < groups) f(group, (int)(LANES == THREADS ? threadIdx.x : threadIdx.x % LANES), LANES);
}

struct DeviceRunner {
    hipStream_t stream;
    const char* me;  // the entry point, for the wording of a failure
    int status = GTSFM_OK;

    // BOUNDS: the __launch_bounds__ of a stage that is launched with fewer threads than it is compiled for
    template <class Tag, int THREADS = STAGE_THREADS, int BOUNDS = THREADS, class F>
    int each(long long n, F f) {
        if (status == GTSFM_OK) hipLaunchKernelGGL((index_stage_kernel<THREADS, BOUNDS, Tag, F>), launch_grid(n, THREADS), dim3(THREADS), 0, stream, n, f);
        return launched(__PRETTY_FUNCTION__);  // names the stage: [Tag = ...]
    }
    template <class Tag, int THREADS, int LANES, class F>
    int group(long long groups, F f) {
        if (status == GTSFM_OK)
            hipLaunchKernelGGL((group_stage_kernel<THREADS, LANES, Tag, F>), launch_grid(groups, THREADS / LANES), dim3(THREADS), 0, stream, groups, f);
        return launched(__PRETTY_FUNCTION__);  // names the stage: [Tag = ...]
    }
    template <class T>
    int scan(T* val, long long n) {
        if (status == GTSFM_OK) hipLaunchKernelGGL(scan_one_workgroup_kernel<T>, dim3(1), dim3(SCAN_THREADS), 0, stream, val, n);
        return launched("scan_one_workgroup_kernel");
    }
    template <class Launch, class Host>
    int block(const char* name, Launch launch, Host) {
        if (status == GTSFM_OK) launch(stream);
        return launched(name);
    }
    template <class T>
    int copy(T* dst, const T* src_dev, size_t count, const char* what) {
        if (status == GTSFM_OK && hipMemcpyAsync(dst, src_dev, count * sizeof(T), hipMemcpyDeviceToHost, stream) != hipSuccess) fail(what);
        return status;
    }
    template <class T>
    int fetch(T* dst, const T* src_dev, size_t count, const char* what) {
        if (copy(dst, src_dev, count, what) == GTSFM_OK && hipStreamSynchronize(stream) != hipSuccess) fail(what);
        return status;
    }
    int zero(void* p, size_t bytes) {
        if (status == GTSFM_OK && hipMemsetAsync(p, 0, bytes, stream) != hipSuccess) fail("hipMemsetAsync");
        return status;
    }

    int launched(const char* name) {
        if (status != GTSFM_OK) return status;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            gtsfm_set_error("kernel launch failed (%s): %s", name, hipGetErrorString(e));
            status = GTSFM_ERR_HIP;  // kept: the stages after it do nothing and the pipeline returns it
        }
        return status;
    }
    void fail(const char* what) {
        gtsfm_set_error("%s: %s failed: %s", me, what, hipGetErrorString(hipGetLastError()));
        status = GTSFM_ERR_HIP;
    }
};

struct HostRunner {
    bool descending, device_lanes;
    int status = GTSFM_OK;

    template <class F>
    void walk(long long n, F f) const {
        if (descending) {
            for (long long i = n - 1; i >= 0; --i) f(i);
        } else {
            for (long long i = 0; i < n; ++i) f(i);
        }
    }
    template <class Tag, int THREADS = STAGE_THREADS, int BOUNDS = THREADS, class F>
    int each(long long n, F f) const {
        walk(n, f);
        return status;
    }
    template <class Tag, int THREADS, int LANES, class F>
    int group(long long groups, F f) const {
        const int lanes = device_lanes ? LANES : 1;
        walk(groups, [&](long long group) { walk(lanes, [&](long long lane) { f(group, (int)lane, lanes); }); });
        return status;
    }
    template <class T>
    int scan(T* val, long long n) const {
        T sum = 0;
        for (long long i = 0; i < n; ++i) {
            const T x = val[i];
            val[i] = sum;
            sum += x;
        }
        val[n] = sum;
        return status;
    }
    template <class Launch, class Host>
    int block(const char*, Launch, Host host) const {
        host(*this);
        return status;
    }
    template <class T>
    int copy(T* dst, const T* src, size_t count, const char* = nullptr) const {
        if (count) memcpy(dst, src, count * sizeof(T));
        return status;
    }
    template <class T>
    int fetch(T* dst, const T* src, size_t count, const char* = nullptr) const {
        return copy(dst, src, count);
    }
    int zero(void* p, size_t bytes) const {
        if (bytes) memset(p, 0, bytes);
        return status;
    }
};

}  // namespace
