// Stand-alone host build of the rotation-averaging solver (gtsfm_amd/csrc/rotation_averaging_kernels.hip: ra_validate and ra_solve, the very
// functions the kernels run), for running it on a CPU and under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-Xarch_host -fsanitize=address,undefined] -c tools/rotation_averaging_host_main.cpp -o main.o
//   hipcc [-fsanitize=address,undefined] main.o -o rotation_averaging_host
//   rotation_averaging_host scene.bin out.bin
//
// scene.bin: int64 {magic, E, N, P, 1 with pair_enable, anchor, chordal_max_iterations, max_outer, max_inner, 0 x 7}, double {chordal_tol,
// delta0, kappa_cg, theta, gradient_tol, 0 x 3}, int32 pair_images[2 E], double rotation[9 E], double weight[E], uint8 pair_enable[E], int64
// problem_row_off[P + 1]. out.bin: double wRi[P N 9], uint8 node_valid[P N], int32 counters[P 8], double costs[P 4].
//
// The solver runs three times. First ONE lane does everything, over a workspace and outputs filled with zeros. Then the device's 256-lane
// partition, the last lane first in every section, over memory filled with 0xFF; the atomics are plain updates here, so the two runs hand
// out the list slots in opposite orders. The outputs must be byte-equal (exit status 2 when they are not). Then every problem of the batch
// is solved ALONE, as the only problem of a call over its own rows, and must give the bytes it gave inside the batch (exit status 4). Exit
// status 3: the input is refused, with the reason on stderr; 1: a bad file. Every input array is a heap allocation of its exact size, so a
// read outside it is a sanitizer report.

#include "../gtsfm_amd/csrc/rotation_averaging_kernels.hip"
#include "host_main_common.h"

namespace {

const long long SCENE_MAGIC = 0x3147564154524d46ll;  // "FMRTAVG1"

struct Scene {
    long long E, N, P, has_enable, anchor, chordal_cap, max_outer, max_inner;
    double chordal_tol, delta0, kappa_cg, theta, gradient_tol;
    int* pair_images;
    double *rotation, *weight;
    uint8_t* pair_enable;
    long long* row_off;
};

bool read_scene(const char* path, Scene& s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    long long head[16];
    double opts[8];
    bool ok = fread(head, 8, 16, f) == 16 && fread(opts, 8, 8, f) == 8 && head[0] == SCENE_MAGIC && ra_sizes_ok(head[1], head[2], head[3]);
    if (ok) {
        s.E = head[1], s.N = head[2], s.P = head[3], s.has_enable = head[4], s.anchor = head[5], s.chordal_cap = head[6], s.max_outer = head[7], s.max_inner = head[8];
        s.chordal_tol = opts[0], s.delta0 = opts[1], s.kappa_cg = opts[2], s.theta = opts[3], s.gradient_tol = opts[4];
        const size_t E = s.E;
        s.pair_images = read_array<int>(f, 2 * E, &ok), s.rotation = read_array<double>(f, 9 * E, &ok), s.weight = read_array<double>(f, E, &ok);
        s.pair_enable = read_array<uint8_t>(f, E, &ok), s.row_off = read_array<long long>(f, s.P + 1, &ok);
    }
    fclose(f);
    return ok;
}

void free_scene(Scene& s) { free(s.pair_images), free(s.rotation), free(s.weight), free(s.pair_enable), free(s.row_off); }

struct Outputs {
    std::vector<double> wri, costs;
    std::vector<uint8_t> node_valid;
    std::vector<int> counters;
};

// 0: done; 3: refused
int run(const Scene& s, int lanes, bool descending, int fill, Outputs& out) {
    const size_t P = s.P, N = s.N;
    fill_vector(out.wri, P * N * 9, fill), fill_vector(out.node_valid, P * N, fill), fill_vector(out.counters, P * 8, fill), fill_vector(out.costs, P * 4, fill);
    if (!(s.anchor >= -1 && (s.anchor < s.N || s.anchor == -1)) || !ra_theta_ok(s.theta)) {
        fprintf(stderr, "refused: the anchor or theta\n");
        return 3;
    }
    const size_t bytes = ra_layout(nullptr, s.E, s.N, s.P).bytes;
    void* ws = filled(bytes, fill);
    RaArgs a{s.pair_images, s.rotation, s.weight, s.has_enable ? s.pair_enable : nullptr, s.row_off, s.E, (int)s.N, (int)s.P, (int)s.anchor, s.chordal_tol, s.delta0,
             s.kappa_cg, s.theta, s.gradient_tol, (int)s.chordal_cap, (int)s.max_outer, (int)s.max_inner, ra_layout(ws, s.E, s.N, s.P), out.wri.data(),
             out.node_valid.data(), out.counters.data(), out.costs.data()};
    for (int i = 0; i < SOLVER_FLAG_WORDS; ++i) a.w.flags[i] = 0;
    const long long n = s.E > s.P ? s.E : s.P;
    for (long long k = 0; k < n; ++k) ra_validate(a, descending ? n - 1 - k : k);
    if (a.w.flags[0] || a.w.flags[1]) {
        fprintf(stderr, "refused: %s\n", a.w.flags[0] ? "a bad pair" : "bad problem offsets");
        free(ws);
        return 3;
    }
    solver_host.lanes = lanes, solver_host.descending = descending ? 1 : 0;
    for (long long k = 0; k < s.P; ++k) ra_solve(a, (int)(descending ? s.P - 1 - k : k));
    free(ws);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]);
        return 1;
    }
    Scene s{};
    if (!read_scene(argv[1], s)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    Outputs first, second;
    int rc = run(s, 1, false, 0x00, first);
    if (rc == 0) rc = run(s, SOLVER_THREADS, true, 0xFF, second);
    if (rc == 0 && !(same(first.wri, second.wri) && same(first.node_valid, second.node_valid) && same(first.counters, second.counters) && same(first.costs, second.costs))) {
        fprintf(stderr, "one lane and %d lanes differ\n", SOLVER_THREADS);
        rc = 2;
    }
    for (long long p = 0; rc == 0 && s.P > 1 && p < s.P; ++p) {  // the problem alone: its rows only, copied to arrays of their exact size
        const long long lo = s.row_off[p], count = s.row_off[p + 1] - lo;
        Scene one = s;
        one.E = count, one.P = 1;
        one.pair_images = copy_of(s.pair_images + 2 * lo, 2 * count), one.rotation = copy_of(s.rotation + 9 * lo, 9 * count);
        one.weight = copy_of(s.weight + lo, count), one.pair_enable = copy_of(s.pair_enable + lo, count), one.row_off = (long long*)malloc(16);
        one.row_off[0] = 0, one.row_off[1] = count;
        Outputs alone;
        rc = run(one, 64, false, 0x55, alone);  // a third lane count
        free_scene(one);
        if (rc == 0 && !(same_slice(first.wri, (size_t)p * s.N * 9, alone.wri) && same_slice(first.node_valid, (size_t)p * s.N, alone.node_valid) &&
                         same_slice(first.counters, (size_t)p * 8, alone.counters) && same_slice(first.costs, (size_t)p * 4, alone.costs))) {
            fprintf(stderr, "problem %lld alone and in the batch differ\n", p);
            rc = 4;
        }
    }
    free_scene(s);
    if (rc) return rc;
    FILE* f = fopen(argv[2], "wb");
    if (!f || !write_vector(f, first.wri) || !write_vector(f, first.node_valid) || !write_vector(f, first.counters) || !write_vector(f, first.costs) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}
