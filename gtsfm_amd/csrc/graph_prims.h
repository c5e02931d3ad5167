// Graph building blocks shared by the tracks, the view graph and 1DSfM (rotation averaging takes the atomic shim only): host/device
// atomics, the workgroup scan and reduce, the single-workgroup prefix sum, the launch grid and the union-find rounds. Everything has
// internal linkage: each translation unit keeps its own instantiation. The header compiles in both passes of hipcc, and the host builds
// under tools/ call the GTSFM_HD functions on a CPU. stage_runner.h, built on this header, launches or walks the stages made of them.
//
// UNION-FIND LABELLING. label[] is a snapshot that a launch only reads, parent[] is the forest the same launch hooks into.
//   init     : parent[v] = label[v] = v, marks / counters / flags cleared (the caller's kernel).
//   hook     : per active edge (u, v): ru = label[u], rv = label[v] (the roots as of the last launch boundary); when they differ,
//              atomicMin(&parent[max(ru, rv)], min(ru, rv)) and the round's flag is raised. The first round also marks both ends as
//              touched. After the launch parent[x] = min(x, every root hooked onto x): a minimum, whatever the order.
//   compress : thread v chases parent[] from v to its root and stores label[v] = parent[v] = root. Only thread v stores parent[v] or
//              label[v] in this launch; a chase that passes through w reads parent[w] before or after thread w's store, and both
//              values lie on w's path to the same root.
//   The host reads the flag words up to the round's after the compress launch (one copy). A round that raised no flag found label[u] == label[v] for every
//   active edge in data published by a launch boundary, so every component carries one label, and since parent[x] <= x that label is
//   the component's smallest node. The host stops there, or fails at UF_MAX_ROUNDS without writing a result.
//
// Invariants:
//   1. parent[x] <= x in every snapshot any thread can observe, fresh or stale: a chase strictly decreases and ends at an x with
//      parent[x] == x.
//   2. Labels only decrease: parent[x] changes by atomicMin, or by thread x storing its own root, which is <= parent[x].
//   3. No kernel waits for another workgroup of its own launch: no spin loop, no decoupled look-back, no flag polled across workgroups.
//      What a later step needs from all workgroups, it gets from a launch boundary.
//   4. The only cross-workgroup traffic inside a launch is the return value of an atomic (a gather cursor). The eight XCD L2s are not
//      coherent with each other and a CU's L1 is never refreshed by another CU's stores, so no kernel reads with a plain load what
//      another workgroup of the same launch stores, except the chase of `compress`, for which invariant 1 makes any mix of old and new
//      values correct.
#pragma once

#include "common.h"

#define GTSFM_HD __host__ __device__ __forceinline__
#define SCAN_THREADS 1024
#define SCAN_ITEMS 4  // values per thread of a scan block
#define SCAN_BLOCK (SCAN_THREADS * SCAN_ITEMS)
#define UF_MAX_ROUNDS 64
#define UF_FLAG_WORDS (8 + UF_MAX_ROUNDS)  // word 0: bad input; words 1 .. 7: the caller's; word 8 + r: round r hooked something

namespace {

// ---- atomics: plain updates in a host build ----

GTSFM_HD int hd_atomic_add(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const int old = *p;
    *p = old + v;
    return old;
#endif
}
GTSFM_HD long long hd_atomic_add(long long* p, long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (long long)atomicAdd((unsigned long long*)p, (unsigned long long)v);
#else
    const long long old = *p;
    *p = old + v;
    return old;
#endif
}
GTSFM_HD void hd_atomic_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// ---- over one workgroup of THREADS lanes, through lds[THREADS] ----

// exclusive scan of one value per thread; *total receives the workgroup's sum
template <int THREADS, class T>
__device__ __forceinline__ T block_exclusive_scan(T x, T* lds, T* total) {
    const int tid = threadIdx.x;
    lds[tid] = x;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const T add = tid >= off ? lds[tid - off] : 0;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    const T excl = lds[tid] - x;
    *total = lds[THREADS - 1];
    __syncthreads();  // lds may be reused
    return excl;
}

// op over one value per thread, by a tree; every thread receives the result
template <int THREADS, class T, class Op>
__device__ __forceinline__ T block_reduce(T x, T* lds, Op op) {
    const int tid = threadIdx.x;
    lds[tid] = x;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) lds[tid] = op(lds[tid], lds[tid + off]);
        __syncthreads();
    }
    const T all = lds[0];
    __syncthreads();  // lds may be reused
    return all;
}

// val[0 .. n) -> its exclusive prefix sum in place, val[n] = the total. Launched as ONE workgroup of SCAN_THREADS, which walks the array
// in blocks of SCAN_BLOCK: the arrays of its callers are a few hundred thousand entries at most, and a single launch keeps the carry in
// a register.
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_one_workgroup_kernel(T* val, long long n) {
    __shared__ T lds[SCAN_THREADS];
    const int tid = threadIdx.x;
    T carry = 0;
    for (long long base = 0; base < n; base += SCAN_BLOCK) {  // n and base are uniform: the barriers stay matched
        const long long at = base + (long long)tid * SCAN_ITEMS;
        T x[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            x[k] = at + k < n ? val[at + k] : 0;
            sum += x[k];
        }
        T total;
        T run = carry + block_exclusive_scan<SCAN_THREADS>(sum, lds, &total);
        carry += total;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (at + k < n) val[at + k] = run;
            run += x[k];
        }
    }
    if (tid == 0) val[n] = carry;
}

// the grid of n indices at per_block each; one block for none, so every launch is valid
inline dim3 launch_grid(long long n, long long per_block) { return dim3((unsigned)(((n > 0 ? n : 1) + per_block - 1) / per_block)); }

// ---- union-find (see the header comment) ----

// the hook of edge (u, v), both inside the node range
GTSFM_HD void uf_hook(int* parent, const int* label, int* mark, int* flags, long long u, long long v, int round) {
    if (round == 0) {
        mark[u] = 1;
        mark[v] = 1;
    }
    const int ru = label[u], rv = label[v];
    if (ru != rv) {
        hd_atomic_min(&parent[ru > rv ? ru : rv], ru < rv ? ru : rv);
        flags[8 + round] = 1;
    }
}

GTSFM_HD void uf_compress(int* parent, int* label, long long v) {
    int x = parent[v];
    for (int p = parent[x]; p != x; p = parent[x]) x = p;  // strictly decreasing (invariant 1)
    label[v] = x;
    parent[v] = x;
}

enum UfOutcome { UF_FIXED_POINT, UF_BAD_INPUT, UF_NO_FIXED_POINT, UF_FAILED };

// The rounds, on the host: hook(r) and compress() run the caller's stages through `run` (a runner of stage_runner.h) and return GTSFM_OK
// or, with the error set, another status; UF_FAILED is that, or a failed readback. *rounds: the rounds completed. The caller words
// UF_BAD_INPUT and UF_NO_FIXED_POINT with its own sizes.
template <class Runner, class Hook, class Compress>
UfOutcome uf_run_rounds(Runner& run, const int* flags, Hook hook, Compress compress, int* rounds) {
    for (*rounds = 0;;) {
        if (*rounds == UF_MAX_ROUNDS) return UF_NO_FIXED_POINT;
        if (hook(*rounds) != GTSFM_OK || compress() != GTSFM_OK) return UF_FAILED;
        int flag[UF_FLAG_WORDS];  // word 0: bad input; word 8 + r: round r hooked
        char what[16];
        snprintf(what, sizeof(what), "round %d", *rounds);
        if (run.fetch(flag, flags, (size_t)(8 + *rounds + 1), what) != GTSFM_OK) return UF_FAILED;
        if (flag[0]) return UF_BAD_INPUT;
        if (!flag[8 + (*rounds)++]) return UF_FIXED_POINT;
    }
}

}  // namespace
