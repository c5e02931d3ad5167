// Stand-alone host build of the translation-recovery solver (gtsfm_amd/csrc/translation_recovery_kernels.hip: trec_validate and trec_solve, the
// very functions the kernels run), for running it on a CPU and under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-Xarch_host -fsanitize=address,undefined] -c tools/translation_recovery_host_main.cpp -o main.o
//   hipcc [-fsanitize=address,undefined] main.o -o translation_recovery_host
//   translation_recovery_host scene.bin out.bin
//
// scene.bin: int64 {magic, E, T, S, N, P, max tracks of a problem, anchor, init_max_iterations, max_outer, max_inner, 0 x 5}, double
// {scale_factor, sigma, huber_k, init_tol, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol, 0 x 7}, int32 pair_images[2 E], double
// world_pair[3 E], uint8 pair_enable[E], int64 track_off[T + 1], int32 image[S], double world_meas[3 S], uint8 meas_enable[S], int64
// problem_row_off[2 (P + 1)]. out.bin, M = N + max tracks: double translation[P M 3], uint8 node_valid[P M], int32 counters[P 8], double
// costs[P 4].
//
// The solver runs three times. First ONE lane does everything, over a workspace and outputs filled with zeros. Then the device's 256-lane
// partition, the last lane first in every section, over memory filled with 0xFF; the atomics are plain updates here, so the two runs hand
// out the list slots in opposite orders. The outputs must be byte-equal (exit status 2 when they are not). Then every problem of the batch
// is solved ALONE, as the only problem of a call over its own rows, and must give the bytes it gave inside the batch (exit status 4). Exit
// status 3: the input is refused, with the reason on stderr; 1: a bad file. Every input array is a heap allocation of its exact size, so a
// read outside it is a sanitizer report.

#include "../gtsfm_amd/csrc/translation_recovery_kernels.hip"
#include "host_main_common.h"

namespace {

const long long SCENE_MAGIC = 0x3143455254524d46ll;  // "FMRTREC1"

struct Scene {
    long long E, T, S, N, P, max_tracks, anchor, init_cap, max_outer, max_inner;
    double scale, sigma, huber_k, init_tol, delta0, kappa_cg, gradient_tol, rel_tol, abs_tol;
    int *pair_images, *image;
    double *world_pair, *world_meas;
    uint8_t *pair_enable, *meas_enable;
    long long *track_off, *row_off;
};

bool read_scene(const char* path, Scene& s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    long long head[16];
    double opts[16];
    bool ok = fread(head, 8, 16, f) == 16 && fread(opts, 8, 16, f) == 16 && head[0] == SCENE_MAGIC && trec_sizes_ok(head[1], head[3], head[4], head[2], head[6], head[5]);
    if (ok) {
        s.E = head[1], s.T = head[2], s.S = head[3], s.N = head[4], s.P = head[5], s.max_tracks = head[6], s.anchor = head[7], s.init_cap = head[8], s.max_outer = head[9];
        s.max_inner = head[10];
        s.scale = opts[0], s.sigma = opts[1], s.huber_k = opts[2], s.init_tol = opts[3], s.delta0 = opts[4], s.kappa_cg = opts[5], s.gradient_tol = opts[6];
        s.rel_tol = opts[7], s.abs_tol = opts[8];
        const size_t E = s.E, S = s.S;
        s.pair_images = read_array<int>(f, 2 * E, &ok), s.world_pair = read_array<double>(f, 3 * E, &ok), s.pair_enable = read_array<uint8_t>(f, E, &ok);
        s.track_off = read_array<long long>(f, s.T + 1, &ok), s.image = read_array<int>(f, S, &ok), s.world_meas = read_array<double>(f, 3 * S, &ok);
        s.meas_enable = read_array<uint8_t>(f, S, &ok), s.row_off = read_array<long long>(f, 2 * (s.P + 1), &ok);
    }
    fclose(f);
    return ok;
}

void free_scene(Scene& s) {
    free(s.pair_images), free(s.world_pair), free(s.pair_enable), free(s.track_off), free(s.image), free(s.world_meas), free(s.meas_enable), free(s.row_off);
}

struct Outputs {
    std::vector<double> translation, costs;
    std::vector<uint8_t> node_valid;
    std::vector<int> counters;
};

// 0: done; 3: refused
int run(const Scene& s, int lanes, bool descending, int fill, Outputs& out) {
    const size_t P = s.P, M = s.N + s.max_tracks;
    fill_vector(out.translation, P * M * 3, fill), fill_vector(out.node_valid, P * M, fill), fill_vector(out.counters, P * 8, fill), fill_vector(out.costs, P * 4, fill);
    if (!(s.anchor >= -1 && (s.anchor < (long long)M || s.anchor == -1)) ||
        !trec_options_ok(s.scale, s.sigma, s.huber_k, s.init_tol, (int)s.init_cap, s.delta0, s.kappa_cg, s.gradient_tol, s.rel_tol, s.abs_tol, (int)s.max_outer, (int)s.max_inner)) {
        fprintf(stderr, "refused: the anchor or an option\n");
        return 3;
    }
    const size_t bytes = trec_layout(nullptr, s.E, s.S, (long long)M, s.P).bytes;
    void* ws = filled(bytes, fill);
    TrecArgs a{s.pair_images, s.world_pair, s.pair_enable, s.track_off, s.image, s.world_meas, s.meas_enable, s.row_off, s.E, s.T, s.S, (int)s.N, (int)s.max_tracks, (int)s.P,
               (int)s.anchor, s.scale, s.sigma, s.huber_k, s.init_tol, s.delta0, s.kappa_cg, s.gradient_tol, s.rel_tol, s.abs_tol, (int)s.init_cap, (int)s.max_outer,
               (int)s.max_inner, trec_layout(ws, s.E, s.S, (long long)M, s.P), out.translation.data(), out.node_valid.data(), out.counters.data(), out.costs.data()};
    for (int i = 0; i < SOLVER_FLAG_WORDS; ++i) a.w.flags[i] = 0;
    const long long n = trec_validate_lanes(s.E, s.S, s.T, s.P);
    for (long long k = 0; k < n; ++k) trec_validate(a, descending ? n - 1 - k : k);
    if (a.w.flags[0] || a.w.flags[1]) {
        fprintf(stderr, "refused: %s\n", a.w.flags[0] ? "a bad pair or measurement" : "bad track or problem offsets");
        free(ws);
        return 3;
    }
    solver_host.lanes = lanes, solver_host.descending = descending ? 1 : 0;
    for (long long k = 0; k < s.P; ++k) trec_solve(a, (int)(descending ? s.P - 1 - k : k));
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
    if (rc == 0 && !(same(first.translation, second.translation) && same(first.node_valid, second.node_valid) && same(first.counters, second.counters) &&
                     same(first.costs, second.costs))) {
        fprintf(stderr, "one lane and %d lanes differ\n", SOLVER_THREADS);
        rc = 2;
    }
    const size_t M = s.N + s.max_tracks;
    for (long long p = 0; rc == 0 && s.P > 1 && p < s.P; ++p) {  // the problem alone: its rows only, copied to arrays of their exact size
        const long long plo = s.row_off[2 * p], pn = s.row_off[2 * p + 2] - plo, tlo = s.row_off[2 * p + 1], tn = s.row_off[2 * p + 3] - tlo;
        const long long mlo = s.track_off[tlo], mn = s.track_off[tlo + tn] - mlo;
        Scene one = s;
        one.E = pn, one.T = tn, one.S = mn, one.P = 1, one.max_tracks = tn;
        one.pair_images = copy_of(s.pair_images + 2 * plo, 2 * pn), one.world_pair = copy_of(s.world_pair + 3 * plo, 3 * pn), one.pair_enable = copy_of(s.pair_enable + plo, pn);
        one.track_off = copy_of(s.track_off + tlo, tn + 1), one.image = copy_of(s.image + mlo, mn), one.world_meas = copy_of(s.world_meas + 3 * mlo, 3 * mn);
        one.meas_enable = copy_of(s.meas_enable + mlo, mn), one.row_off = (long long*)malloc(32);
        for (long long j = 0; j <= tn; ++j) one.track_off[j] -= mlo;
        one.row_off[0] = 0, one.row_off[1] = 0, one.row_off[2] = pn, one.row_off[3] = tn;
        Outputs alone;
        rc = run(one, 64, false, 0x55, alone);  // a third lane count
        free_scene(one);
        const size_t m1 = s.N + tn;  // the nodes it has alone: the first m1 of its M in the batch, the others NaN / 0 there
        if (rc == 0 && !(same_slice(first.translation, (size_t)p * M * 3, alone.translation) && same_slice(first.node_valid, (size_t)p * M, alone.node_valid) &&
                         same_slice(first.counters, (size_t)p * 8, alone.counters) && same_slice(first.costs, (size_t)p * 4, alone.costs))) {
            fprintf(stderr, "problem %lld alone and in the batch differ\n", p);
            rc = 4;
        }
        for (size_t k = m1; rc == 0 && k < M; ++k)
            if (first.node_valid[p * M + k] != 0) rc = 4;
    }
    free_scene(s);
    if (rc) return rc;
    FILE* f = fopen(argv[2], "wb");
    if (!f || !write_vector(f, first.translation) || !write_vector(f, first.node_valid) || !write_vector(f, first.counters) || !write_vector(f, first.costs) ||
        fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}
