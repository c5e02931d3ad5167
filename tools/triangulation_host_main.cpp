// Stand-alone host build of the triangulation kernels' per-track arithmetic (the TRI_HD functions of
// gtsfm_amd/csrc/triangulation_kernels.hip), for running it on a CPU and under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-Xarch_host -fsanitize=address,undefined] -c tools/triangulation_host_main.cpp -o main.o
//   hipcc [-fsanitize=address,undefined] main.o -o triangulation_host
//   triangulation_host scene.bin out.bin
//
// scene.bin: int64 {magic, T, S, num_images, mode, num_hypotheses, seed, 0}, double {threshold, min_angle_deg}, int64 track_off[T + 1],
// int32 image[S], float uv[2 S], double cameras[17 num_images]. out.bin: two copies (one per lane partition, see below) of double
// point[3 T], double avg_error[T], int32 exit_code[T], uint8 inlier_mask[S], int32 stats[4 T].
//
// The stages are the device call's own (tri_triangulate_stages), walked by the HostRunner of gtsfm_amd/csrc/stage_runner.h. They run
// twice: ascending with one lane per group (select: one lane per track; hypothesis: min(ceil(cap / 256), 2048) lanes, grid-stride) over a
// zeroed workspace, and descending with the device's partition (256 lanes per track; a grid of that many groups x 256 lanes, the last
// lane first) over a workspace filled with 0xFF. The two outputs must be byte-equal: exit status 2 when they are not, 3 when the call
// refuses its input (an error flag of the device call; nothing written), with the reason on stderr, 1 for a bad file. Every input array is
// a heap allocation of its exact size, so a read outside it is a sanitizer report.

#include "../gtsfm_amd/csrc/triangulation_kernels.hip"
#include "host_main_common.h"

namespace {

const long long SCENE_MAGIC = 0x3149525453464754ll;  // "TGFSTRI1"

struct Scene {
    long long num_tracks, total, num_images, mode, num_hyp;
    unsigned long long seed;
    double threshold, min_angle;
    long long* track_off;
    int* image;
    float* uv;
    double* cams;
};

bool read_scene(const char* path, Scene& s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    long long head[8];
    double opts[2];
    bool ok = fread(head, 8, 8, f) == 8 && fread(opts, 8, 2, f) == 2 && head[0] == SCENE_MAGIC && head[1] >= 0 && head[2] >= 0 && head[3] >= 0 &&
              head[1] < (1ll << 31) && head[2] < (1ll << 31) && head[3] < (1ll << 31);
    if (ok) {
        s.num_tracks = head[1];
        s.total = head[2];
        s.num_images = head[3];
        s.mode = head[4];
        s.num_hyp = head[5];
        s.seed = (unsigned long long)head[6];
        s.threshold = opts[0];
        s.min_angle = opts[1];
        s.track_off = read_array<long long>(f, (size_t)s.num_tracks + 1, &ok);
        s.image = read_array<int>(f, (size_t)s.total, &ok);
        s.uv = read_array<float>(f, 2 * (size_t)s.total, &ok);
        s.cams = read_array<double>(f, 17 * (size_t)s.num_images, &ok);
    }
    fclose(f);
    return ok;
}

struct Outputs {
    std::vector<double> point, avg;
    std::vector<int> code, stats;
    std::vector<uint8_t> mask;
    Outputs(const Scene& s) : point(3 * s.num_tracks, NAN), avg(s.num_tracks, NAN), code(s.num_tracks, 0), stats(4 * s.num_tracks, 0), mask(s.total, 0) {}
    bool same(const Outputs& o) const {
        auto eq = [](const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; };
        return eq(point.data(), o.point.data(), point.size() * 8) && eq(avg.data(), o.avg.data(), avg.size() * 8) &&
               eq(code.data(), o.code.data(), code.size() * 4) && eq(stats.data(), o.stats.data(), stats.size() * 4) &&
               eq(mask.data(), o.mask.data(), mask.size());
    }
    bool write(FILE* f) const {
        auto put = [&](const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; };
        return put(point.data(), point.size() * 8) && put(avg.data(), avg.size() * 8) && put(code.data(), code.size() * 4) && put(mask.data(), mask.size()) &&
               put(stats.data(), stats.size() * 4);
    }
};

// the call's stages over a workspace filled with `fill`: the pipeline's status
int run(const Scene& s, HostRunner runner, int fill, Outputs& out) {
    const int mode = (int)s.mode;
    const long long max_hyp = mode == TRI_NO_RANSAC ? 0 : s.num_hyp;
    void* base = filled(tri_layout(nullptr, s.num_tracks, s.total, max_hyp).bytes, fill);
    const TriCall c{s.track_off, s.image, s.uv, s.num_tracks, s.total, s.cams, (int)s.num_images, mode, s.threshold, s.min_angle, max_hyp, s.seed, out.point.data(),
                    out.avg.data(), out.code.data(), out.mask.data(), out.stats.data()};
    const int status = tri_triangulate_stages(runner, "triangulation_host", c, tri_layout(base, s.num_tracks, s.total, max_hyp));
    free(base);
    return status;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]);
        return 1;
    }
    Scene s;
    if (!read_scene(argv[1], s)) {
        fprintf(stderr, "%s: not a scene file\n", argv[1]);
        return 1;
    }
    if (s.mode < TRI_NO_RANSAC || s.mode > TRI_TOPK || !(s.threshold > 0.0) || (s.mode != TRI_NO_RANSAC && s.num_hyp < 0)) {
        fprintf(stderr, "%s: options outside the device call's domain\n", argv[1]);
        return 1;
    }
    Outputs serial(s), device(s);
    int status = 0;
    if (s.num_tracks > 0) {
        const int first = run(s, HostRunner{false, false}, 0x00, serial), second = run(s, HostRunner{true, true}, 0xFF, device);
        status = first != second ? 2 : (first != GTSFM_OK ? refused(first) : 0);
    }
    if (status == 0 && !serial.same(device)) {
        fprintf(stderr, "the outputs depend on the lane partition or on what the workspace held\n");
        status = 2;
    }
    if (status == 0) {
        FILE* f = fopen(argv[2], "wb");
        if (!f || !serial.write(f) || !device.write(f)) status = 1;
        if (f) fclose(f);
    }
    free(s.track_off);
    free(s.image);
    free(s.uv);
    free(s.cams);
    return status;
}
