// Stand-alone host build of the view-graph kernels' per-index functions (the GTSFM_HD functions of gtsfm_amd/csrc/view_graph_kernels.hip: the
// adjacency, the merge of two neighbour lists, the cycle error, the per-edge aggregate, the component labelling), for running them on a CPU
// and under the host sanitizers:
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
// The stages are the device calls', each a loop over the indices its kernel covers, with the prefix sums done by a plain loop. They run
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

// 0: done; 3: refused
int run(const Scene& s, bool descending, int fill, Outputs& out) {
    const long long E = s.num_edges, N = s.num_images;
    fill_vector(out.num_triplets, E, fill), fill_vector(out.aggregate, E, fill), fill_vector(out.keep, E, fill), fill_vector(out.counts, 8, fill);
    fill_vector(out.node_mask, N, fill), fill_vector(out.pair_keep, E, fill), fill_vector(out.component_counts, 8, fill);
    out.triplets.clear(), out.cycle_error.clear(), out.total = 0;
    if (E > 0) {
        VgGraph g{s.pair_images, s.rotation, s.has_enable ? s.enable : nullptr, E, (int)N, vg_layout(nullptr, E, N, 0)};
        void* fixed = filled(g.w.bytes, fill);
        g.w = vg_layout(fixed, E, N, 0);
        const long long init_n = N + 1 > VG_FLAG_WORDS ? N + 1 : VG_FLAG_WORDS;
        walk(init_n, descending, [&](long long i) { vg_init(g, i); });
        walk(E, descending, [&](long long i) { vg_edge_degree(g, i); });
        exclusive_scan(g.w.row_off, N);
        walk(E, descending, [&](long long i) { vg_edge_fill(g, i); });
        walk(2 * E, descending, [&](long long i) { vg_slot_rank(g, i); });
        if (g.w.flags[0] || g.w.flags[1]) {
            fprintf(stderr, "refused: %s\n", g.w.flags[0] ? "a bad pair" : "a duplicate edge");
            free(fixed);
            return 3;
        }
        walk(2 * E, descending, [&](long long i) { vg_slot_triplets(g, i, false, nullptr, nullptr); });
        exclusive_scan(g.w.seg_off, 2 * E);
        exclusive_scan(g.w.trip_off, 2 * E);
        const long long total = g.w.trip_off[2 * E];
        if (g.w.seg_off[2 * E] != 3 * total || total >= VG_MAX_TRIPLETS) {
            fprintf(stderr, "refused: %lld list entries for %lld triplets\n", g.w.seg_off[2 * E], total);
            free(fixed);
            return 3;
        }
        // the device lays the error lists behind the fixed part of the same workspace
        const size_t fixed_bytes = g.w.fixed_bytes;
        void* whole = filled(vg_layout(nullptr, E, N, total).bytes, fill);
        memcpy(whole, fixed, fixed_bytes);
        free(fixed);
        g.w = vg_layout(whole, E, N, total);
        out.total = total;
        fill_vector(out.triplets, 3 * total, fill), fill_vector(out.cycle_error, total, fill);
        walk(2 * E, descending, [&](long long i) { vg_slot_triplets(g, i, true, out.triplets.data(), out.cycle_error.data()); });
        const int lanes = descending ? VG_WAVE : 1;
        walk(E, descending, [&](long long e) {
            walk(lanes, descending, [&](long long lane) {
                vg_edge_aggregate(g, e, (int)lane, lanes, (int)s.criterion, s.threshold, out.num_triplets.data(), out.aggregate.data(), out.keep.data());
            });
        });
        memset(out.counts.data(), 0, 8 * sizeof(int));  // vg_filter_counts_kernel: integer sums and a maximum over the rows
        out.counts[2] = (int)total;
        walk(E, descending, [&](long long e) {
            out.counts[0] += g.w.input[e] ? 1 : 0, out.counts[1] += out.keep[e] ? 1 : 0;
            out.counts[3] = out.num_triplets[e] > out.counts[3] ? out.num_triplets[e] : out.counts[3];
        });
        free(whole);
    } else {
        memset(out.counts.data(), 0, 8 * sizeof(int));
    }

    // the largest component of the kept edges
    void* ws = filled(vg_cc_layout(nullptr, N).bytes, fill);
    VgComponents c = vg_cc_layout(ws, N);
    c.pair_images = s.pair_images, c.pair_enable = out.keep.data(), c.num_edges = E, c.num_images = (int)N;
    const long long init_n = N > VG_FLAG_WORDS ? N : VG_FLAG_WORDS;
    walk(init_n, descending, [&](long long i) { vg_cc_init(c, i); });
    for (int rounds = 0; E > 0;) {
        if (rounds == UF_MAX_ROUNDS) {
            fprintf(stderr, "refused: no fixed point after %d rounds\n", rounds);
            free(ws);
            return 3;
        }
        walk(E, descending, [&](long long i) { vg_cc_hook(c, i, rounds); });
        walk(N, descending, [&](long long i) { uf_compress(c.parent, c.label, i); });
        if (c.flags[0]) {
            fprintf(stderr, "refused: a bad pair\n");
            free(ws);
            return 3;
        }
        if (!c.flags[8 + rounds++]) break;
    }
    memset(out.component_counts.data(), 0, 8 * sizeof(int));
    if (E > 0) {
        walk(N, descending, [&](long long i) { vg_cc_node_count(c, i); });
    }
    vg_u64 largest = 0, bid = 0;  // vg_cc_summary_kernel: the largest size and the roots, the winning bid, the component's edges
    walk(N, descending, [&](long long v) {
        const vg_u64 size = c.cnt[v] > 0 ? (vg_u64)c.cnt[v] : 0;
        out.component_counts[2] += size ? 1 : 0;
        largest = size > largest ? size : largest;
    });
    if (largest) walk(E, descending, [&](long long e) {
        const vg_u64 b = vg_cc_edge_bid(c, e, (int)largest);
        bid = b > bid ? b : bid;
    });
    const vg_u64 best = largest ? (largest << 32) | bid : 0;
    *c.best = best;
    out.component_counts[0] = (int)(best >> 32);
    walk(E, descending, [&](long long e) { out.component_counts[1] += vg_cc_edge_kept(c, e, vg_cc_root_of_key(c, best)) ? 1 : 0; });
    walk(N, descending, [&](long long i) { vg_cc_write_node(c, i, out.node_mask.data()); });
    walk(E, descending, [&](long long i) { vg_cc_write_edge(c, i, out.pair_keep.data()); });
    free(ws);
    return 0;
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
    int rc = run(s, false, 0x00, first);
    if (rc == 0) rc = run(s, true, 0xFF, second);
    free(s.pair_images), free(s.rotation), free(s.enable);
    if (rc) return rc;
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
