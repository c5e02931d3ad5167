// Stand-alone host build of the global bundle adjustment (gtsfm_amd/csrc/global_ba_kernels.hip: gba_validate and gba_solve, the very functions
// the kernels run), for running it on a CPU and under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-Xarch_host -fsanitize=address,undefined] -c tools/global_ba_host_main.cpp -o main.o
//   hipcc [-fsanitize=address,undefined] main.o -o global_ba_host
//   global_ba_host scene.bin out.bin
//
// scene.bin: int64 {magic, N, T, S, P, max tracks of a problem, anchor, min_track_length, max_iterations, max_inner, 0 x 6}, double
// {measurement_sigma, huber_k, reproj_error_threshold, rel_tol, abs_tol, cg_forcing, 0 x 10}, double cameras[17 N], int64 track_off[T + 1],
// int32 image[S], float uv[2 S], double point[3 T], uint8 track_enable[T], uint8 meas_enable[S], int64 problem_off[P + 1]. out.bin, M = N + max
// tracks: double cameras_out[P N 17], double point_out[T 3], double reproj_error[S], uint8 track_valid[T], uint8 camera_kept[P N], uint8
// node_valid[P M], int32 counters[P 8], double costs[P 4].
//
// The solver runs three times. First ONE lane does everything, over a workspace and outputs filled with zeros. Then the device's 256-lane
// partition, the last lane first in every section, over memory filled with 0xFF; the atomics are plain updates here, so the two runs hand
// out the list slots in opposite orders. The outputs must be byte-equal (exit status 2 when they are not). Then every problem of the batch
// is solved ALONE, as the only problem of a call over its own tracks, and must give the bytes it gave inside the batch (exit status 4). Exit
// status 3: the input is refused, with the reason on stderr; 1: a bad file. Every input array is a heap allocation of its exact size, so a
// read outside it is a sanitizer report.

#include "../gtsfm_amd/csrc/global_ba_kernels.hip"
#include "host_main_common.h"

namespace {

const long long SCENE_MAGIC = 0x3141424c47524d46ll;  // "FMRGLBA1"

struct Scene {
    long long N, T, S, P, max_tracks, anchor, min_len, max_iterations, max_inner;
    double sigma, huber_k, threshold, rel_tol, abs_tol, cg_forcing;
    double *cameras, *point;
    long long *track_off, *problem_off;
    int* image;
    float* uv;
    uint8_t *track_enable, *meas_enable;
};

bool read_scene(const char* path, Scene& s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    long long head[16];
    double opts[16];
    bool ok = fread(head, 8, 16, f) == 16 && fread(opts, 8, 16, f) == 16 && head[0] == SCENE_MAGIC && gba_sizes_ok(head[3], head[1], head[2], head[5], head[4]);
    if (ok) {
        s.N = head[1], s.T = head[2], s.S = head[3], s.P = head[4], s.max_tracks = head[5], s.anchor = head[6], s.min_len = head[7], s.max_iterations = head[8];
        s.max_inner = head[9];
        s.sigma = opts[0], s.huber_k = opts[1], s.threshold = opts[2], s.rel_tol = opts[3], s.abs_tol = opts[4], s.cg_forcing = opts[5];
        const size_t N = s.N, T = s.T, S = s.S;
        s.cameras = read_array<double>(f, 17 * N, &ok), s.track_off = read_array<long long>(f, T + 1, &ok), s.image = read_array<int>(f, S, &ok);
        s.uv = read_array<float>(f, 2 * S, &ok), s.point = read_array<double>(f, 3 * T, &ok), s.track_enable = read_array<uint8_t>(f, T, &ok);
        s.meas_enable = read_array<uint8_t>(f, S, &ok), s.problem_off = read_array<long long>(f, s.P + 1, &ok);
    }
    fclose(f);
    return ok;
}

void free_scene(Scene& s, bool cameras_too) {
    if (cameras_too) free(s.cameras);
    free(s.track_off), free(s.image), free(s.uv), free(s.point), free(s.track_enable), free(s.meas_enable), free(s.problem_off);
}

struct Outputs {
    std::vector<double> cameras, point, reproj, costs;
    std::vector<uint8_t> track_valid, camera_kept, node_valid;
    std::vector<int> counters;
};

// 0: done; 3: refused
int run(const Scene& s, int lanes, bool descending, int fill, Outputs& out) {
    const size_t P = s.P, N = s.N, M = s.N + s.max_tracks, T = s.T, S = s.S;
    fill_vector(out.cameras, P * N * 17, fill), fill_vector(out.point, T * 3, fill), fill_vector(out.reproj, S, fill), fill_vector(out.track_valid, T, fill);
    fill_vector(out.camera_kept, P * N, fill), fill_vector(out.node_valid, P * M, fill), fill_vector(out.counters, P * 8, fill), fill_vector(out.costs, P * 4, fill);
    if (!(s.anchor >= -1 && (s.anchor < s.N || s.anchor == -1)) ||
        !gba_options_ok((int)s.min_len, s.sigma, s.huber_k, s.threshold, s.rel_tol, s.abs_tol, s.cg_forcing, (int)s.max_iterations, (int)s.max_inner)) {
        fprintf(stderr, "refused: the anchor or an option\n");
        return 3;
    }
    const size_t bytes = gba_layout(nullptr, s.S, (long long)M, s.P).bytes;
    void* ws = filled(bytes, fill);
    GbaArgs a{s.cameras, s.track_off, s.image, s.uv, s.point, s.track_enable, s.meas_enable, s.problem_off, s.T, s.S, (int)s.N, (int)s.max_tracks, (int)s.P, (int)s.anchor,
              (int)s.min_len, s.sigma, s.huber_k, s.threshold, s.rel_tol, s.abs_tol, s.cg_forcing, (int)s.max_iterations, (int)s.max_inner,
              gba_layout(ws, s.S, (long long)M, s.P), out.cameras.data(), out.point.data(), out.reproj.data(), out.track_valid.data(), out.camera_kept.data(),
              out.node_valid.data(), out.counters.data(), out.costs.data()};
    for (int i = 0; i < SOLVER_FLAG_WORDS; ++i) a.w.flags[i] = 0;
    const long long n = gba_validate_lanes(s.T, s.P);
    for (long long k = 0; k < n; ++k) gba_validate(a, descending ? n - 1 - k : k);
    if (a.w.flags[0] || a.w.flags[1]) {
        fprintf(stderr, "refused: %s\n", a.w.flags[0] ? "bad track offsets" : "bad problem offsets");
        free(ws);
        return 3;
    }
    solver_host.lanes = lanes, solver_host.descending = descending ? 1 : 0;
    for (long long k = 0; k < s.P; ++k) gba_solve(a, (int)(descending ? s.P - 1 - k : k));
    free(ws);
    return 0;
}

bool same_outputs(const Outputs& a, const Outputs& b) {
    return same(a.cameras, b.cameras) && same(a.point, b.point) && same(a.reproj, b.reproj) && same(a.track_valid, b.track_valid) && same(a.camera_kept, b.camera_kept) &&
           same(a.node_valid, b.node_valid) && same(a.counters, b.counters) && same(a.costs, b.costs);
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
    if (rc == 0 && !same_outputs(first, second)) {
        fprintf(stderr, "one lane and %d lanes differ\n", SOLVER_THREADS);
        rc = 2;
    }
    const size_t N = s.N, M = s.N + s.max_tracks;
    for (long long p = 0; rc == 0 && s.P > 1 && p < s.P; ++p) {  // the problem alone: its tracks only, copied to arrays of their exact size
        const long long tlo = s.problem_off[p], tn = s.problem_off[p + 1] - tlo, mlo = s.track_off[tlo], mn = s.track_off[tlo + tn] - mlo;
        Scene one = s;
        one.T = tn, one.S = mn, one.P = 1, one.max_tracks = tn;
        one.track_off = copy_of(s.track_off + tlo, tn + 1), one.image = copy_of(s.image + mlo, mn), one.uv = copy_of(s.uv + 2 * mlo, 2 * mn);
        one.point = copy_of(s.point + 3 * tlo, 3 * tn), one.track_enable = copy_of(s.track_enable + tlo, tn), one.meas_enable = copy_of(s.meas_enable + mlo, mn);
        one.problem_off = (long long*)malloc(16);
        for (long long j = 0; j <= tn; ++j) one.track_off[j] -= mlo;
        one.problem_off[0] = 0, one.problem_off[1] = tn;
        Outputs alone;
        rc = run(one, 64, false, 0x55, alone);  // a third lane count
        free_scene(one, false);
        if (rc == 0 && !(same_slice(first.cameras, (size_t)p * N * 17, alone.cameras) && same_slice(first.point, (size_t)tlo * 3, alone.point) &&
                         same_slice(first.reproj, (size_t)mlo, alone.reproj) && same_slice(first.track_valid, (size_t)tlo, alone.track_valid) &&
                         same_slice(first.camera_kept, (size_t)p * N, alone.camera_kept) && same_slice(first.node_valid, (size_t)p * M, alone.node_valid) &&
                         same_slice(first.counters, (size_t)p * 8, alone.counters) && same_slice(first.costs, (size_t)p * 4, alone.costs))) {
            fprintf(stderr, "problem %lld alone and in the batch differ\n", p);
            rc = 4;
        }
        for (size_t k = N + tn; rc == 0 && k < M; ++k)
            if (first.node_valid[p * M + k] != 0) rc = 4;
    }
    free_scene(s, true);
    if (rc) return rc;
    FILE* f = fopen(argv[2], "wb");
    if (!f || !write_vector(f, first.cameras) || !write_vector(f, first.point) || !write_vector(f, first.reproj) || !write_vector(f, first.track_valid) ||
        !write_vector(f, first.camera_kept) || !write_vector(f, first.node_valid) || !write_vector(f, first.counters) || !write_vector(f, first.costs) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}
