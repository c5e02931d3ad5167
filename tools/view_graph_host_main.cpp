// Stand-alone host build of the two view-graph calls (vg_cycle_filter_stages and vg_largest_component_stages of
// gtsfm_amd/csrc/view_graph_kernels.hip: the very stage sequences the device calls launch, over the same GTSFM_HD per-index functions), for
// running them on a CPU and under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off [-Xarch_host -fsanitize=address,undefined] -c tools/view_graph_host_main.cpp -o main.o
//   hipcc [-fsanitize=address,undefined] main.o -o view_graph_host
//   view_graph_host scene.bin out.bin
//
// scene.bin: int64 {magic, E, num_images, 1 with pair_enable, criterion, 0, 0, 0}, double {error_threshold, 0 x 7}, int32 pair_images[2 E],
// double rotation[9 E], uint8 pair_enable[E]. out.bin: two copies (see below) of int32 num_triplets[E], double aggregate_error[E],
// uint8 keep[E], int32 counts[8], int64 T, int32 triplets[3 T], double cycle_error[T], then the largest component of the kept edges:
// uint8 node_mask[num_images], uint8 pair_keep[E], int32 counts[8].
//
// The stages are the device calls' own, walked by the HostRunner of gtsfm_amd/csrc/stage_runner.h: each a loop over the indices its kernel
// covers, the prefix sums and the block-cooperative kernels by the plain loops written next to them. They run
// twice. First every stage walks its indices in ASCENDING order and ONE lane does the whole aggregate of an edge, over a workspace and
// outputs filled with zeros. Then every stage walks its indices in DESCENDING order and the aggregate of an edge is done by 64 lanes, the
// last lane first, over memory filled with 0xFF. The atomics are plain updates here, so the two runs hand out the list slots in opposite
// orders. The two outputs must be byte-equal (exit status 2 when they are not): neither the order of the indices, nor the lane partition,
// nor what the memory held may matter. Exit status 3: the input is refused (a bad pair, a duplicate edge, no fixed point of the labelling),
// with the reason on stderr; 1: a bad file.
// Every input array is a heap allocation of its exact size, so a read outside it is a sanitizer report.

#include "../gtsfm_amd/csrc/view_graph_kernels.hip"
#include "host_main_common.h"

namespace {

const long long SCENE_MAGIC = 0x3148505247574956ll;  // "VIWGRPH1"

struct Scene {
    long long num_edges, num_images, has_enable, criterion;
    double threshold;
    int* pair_images;
    double* rotation;
    uint8_t* enable;
};

bool read_scene(const char* path, Scene& s) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    long long head[8];
    double opts[8];
    bool ok = fread(head, 8, 8, f) == 8 && fread(opts, 8, 8, f) == 8 && head[0] == SCENE_MAGIC && head[1] >= 0 && head[1] < VG_MAX_EDGES && head[2] >= 0 &&
              head[2] < VG_MAX_IMAGES && (head[4] == 0 || head[4] == 1);
    if (ok) {
        s.num_edges = head[1], s.num_images = head[2], s.has_enable = head[3], s.criterion = head[4], s.threshold = opts[0];
        s.pair_images = read_array<int>(f, 2 * (size_t)s.num_edges, &ok);
        s.rotation = read_array<double>(f, 9 * (size_t)s.num_edges, &ok);
        s.enable = read_array<uint8_t>(f, (size_t)s.num_edges, &ok);
    }
    fclose(f);
    return ok;
}

struct Outputs {
    std::vector<int> num_triplets, counts, triplets, component_counts;
    std::vector<double> aggregate, cycle_error;
    std::vector<uint8_t> keep, node_mask, pair_keep;
    long long total = 0;
};

// Both calls' stages over memory filled with `fill`: the pipeline's status. The triplet capacity is found the way ViewGraphEngine finds
// it: a call that only counts (capacity 0), then one with the capacity it reported.
int run(const Scene& s, HostRunner runner, int fill, Outputs& out) {
    const char* me = "view_graph_host";
    const long long E = s.num_edges, N = s.num_images;
    fill_vector(out.num_triplets, E, fill), fill_vector(out.aggregate, E, fill), fill_vector(out.keep, E, fill), fill_vector(out.counts, 8, fill);
    fill_vector(out.node_mask, N, fill), fill_vector(out.pair_keep, E, fill), fill_vector(out.component_counts, 8, fill);
    int status = GTSFM_OK;
    long long capacity = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        GTSFM_CHECK_ARG(gtsfm_view_graph_workspace_bytes(E, N, capacity) > 0, "%s: sizes out of range (%lld triplets)", me, capacity);
        void* ws = filled(vg_layout(nullptr, E, N, capacity).bytes, fill);
        const VgGraph g{s.pair_images, s.rotation, s.has_enable ? s.enable : nullptr, E, (int)N, vg_layout(ws, E, N, capacity)};
        fill_vector(out.triplets, 3 * capacity, fill), fill_vector(out.cycle_error, capacity, fill);
        status = vg_cycle_filter_stages(runner, me, g, (int)s.criterion, s.threshold, capacity, out.num_triplets.data(), out.aggregate.data(), out.keep.data(),
                                        out.counts.data(), out.triplets.data(), out.cycle_error.data(), &out.total);
        free(ws);
        if (status != GTSFM_ERR_WORKSPACE || out.total <= capacity) break;
        capacity = out.total;
    }
    if (status != GTSFM_OK) return status;

    // the largest component of the kept edges
    void* ws = filled(vg_cc_layout(nullptr, N).bytes, fill);
    VgComponents c = vg_cc_layout(ws, N);
    c.pair_images = s.pair_images, c.pair_enable = out.keep.data(), c.num_edges = E, c.num_images = (int)N;
    status = vg_largest_component_stages(runner, me, c, out.node_mask.data(), out.pair_keep.data(), out.component_counts.data());
    free(ws);
    return status;
}

bool write_outputs(FILE* f, const Outputs& o) {
    return write_vector(f, o.num_triplets) && write_vector(f, o.aggregate) && write_vector(f, o.keep) && write_vector(f, o.counts) && fwrite(&o.total, 8, 1, f) == 1 &&
           write_vector(f, o.triplets) && write_vector(f, o.cycle_error) && write_vector(f, o.node_mask) && write_vector(f, o.pair_keep) &&
           write_vector(f, o.component_counts);
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
    int status = run(s, HostRunner{false, false}, 0x00, first);
    if (status == GTSFM_OK) status = run(s, HostRunner{true, true}, 0xFF, second);
    free(s.pair_images), free(s.rotation), free(s.enable);
    if (status != GTSFM_OK) return refused(status);
    FILE* f = fopen(argv[2], "wb");
    if (!f || !write_outputs(f, first) || !write_outputs(f, second) || fclose(f) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    const bool equal = same(first.num_triplets, second.num_triplets) && same(first.aggregate, second.aggregate) && same(first.keep, second.keep) &&
                       same(first.counts, second.counts) && first.total == second.total && same(first.triplets, second.triplets) &&
                       same(first.cycle_error, second.cycle_error) && same(first.node_mask, second.node_mask) && same(first.pair_keep, second.pair_keep) &&
                       same(first.component_counts, second.component_counts);
    if (!equal) {
        fprintf(stderr, "the two runs differ\n");
        return 2;
    }
    return 0;
}
