// Stand-alone host build of the solvers' shared scaffold (gtsfm_amd/csrc/problem_solver.h), for running it on a CPU and under the host
// sanitizers; built like the other tools/*_host_main.cpp. It takes no argument.
//
// solver_scan, solver_tree (through the two per-node reductions as well), solver_build_lists and solver_component run on tiny inputs
// under three lane settings -- one lane over zeroed memory, 256 lanes last lane first over 0xFF, 64 lanes over 0x55 -- and every output is
// compared, byte for byte, with a plain single-threaded loop written here. Exit status 2: a difference, named on stderr.

#include "../gtsfm_amd/csrc/problem_solver.h"
#include "host_main_common.h"

#include <algorithm>
#include <array>

namespace {

int failures = 0;

template <class T>
void expect(const char* what, const T* got, const std::vector<T>& want) {
    if (want.empty() || memcmp(got, want.data(), want.size() * sizeof(T)) == 0) return;
    fprintf(stderr, "%s differs with %d lanes%s\n", what, solver_host.lanes, solver_host.descending ? ", descending" : "");
    ++failures;
}

void check_scan(int n, int fill) {
    std::vector<int> val, want(n + 1, 0);
    std::vector<long long> lanebuf;
    fill_vector(val, n + 1, fill), fill_vector(lanebuf, SOLVER_THREADS, fill);
    for (int i = 0; i < n; ++i) val[i] = (7 * i + 3) % 5, want[i + 1] = want[i] + val[i];
    solver_scan(val.data(), n, lanebuf.data());
    expect("scan", val.data(), want);
}

double pairwise(const double* t, int len, bool take_max) {  // the tree, by halves
    if (len == 1) return t[0];
    const double x = pairwise(t, len / 2, take_max), y = pairwise(t + len / 2, len / 2, take_max);
    return take_max ? (x > y ? x : y) : x + y;
}

// n nodes of 3 numbers each: the dot product and the infinity norm through the tree padded to p2
void check_tree(int n, int fill) {
    SolverGraph g{};
    g.n = n, g.p2 = 1;
    while (g.p2 < n) g.p2 *= 2;
    std::vector<double> t, x(3 * n), y(3 * n), dots(g.p2, 0.0), maxs(g.p2, 0.0);
    fill_vector(t, g.p2, fill);
    g.t = t.data();
    for (int i = 0; i < 3 * n; ++i) x[i] = 0.1 * (i + 1) * (i % 2 ? -1 : 1), y[i] = 1.0 / (i + 3);
    for (int c = 0; c < n; ++c) {
        dots[c] = (x[3 * c] * y[3 * c] + x[3 * c + 1] * y[3 * c + 1]) + x[3 * c + 2] * y[3 * c + 2];
        maxs[c] = std::max(std::max(fabs(x[3 * c]), fabs(x[3 * c + 1])), fabs(x[3 * c + 2]));
    }
    const double dot = solver_dot_nodes(g, x.data(), y.data(), 3), inf = solver_inf_norm(g, x.data(), 3);
    expect("tree sum", &dot, std::vector<double>{pairwise(dots.data(), g.p2, false)});
    expect("tree max", &inf, std::vector<double>{pairwise(maxs.data(), g.p2, true)});
}

struct Row {
    int a, b, valid;
};

// the lists of `rows` over `nodes` node ids, then the component of `anchor`
void check_graph(const std::vector<Row>& rows, int nodes, int anchor, int fill) {
    const int R = (int)rows.size();
    WorkspaceCarver size{nullptr, 0};
    solver_carve(size, R, nodes, 1);
    void* ws = filled(size.used, fill);
    WorkspaceCarver carve{ws, 0};
    SolverGraph g = solver_slice(solver_carve(carve, R, nodes, 1), 0, nodes, 0);
    solver_clear(g, nodes, 0, 1);
    int entries = -1;
    const int first = solver_build_lists(
        g, nodes, R, [&](int l, int* a, int* b) { *a = rows[l].a, *b = rows[l].b; }, [&](int l) { return rows[l].valid != 0; }, &entries);

    std::vector<std::vector<std::array<int, 3>>> lists(nodes);  // (neighbour, row, the node is the row's a)
    std::vector<int> off(1, 0), nbr, row_bit, want_first(1, R);
    for (int l = R - 1; l >= 0; --l)
        if (rows[l].valid) want_first[0] = l, lists[rows[l].a].push_back({rows[l].b, l, 1}), lists[rows[l].b].push_back({rows[l].a, l, 0});
    for (auto& list : lists) {
        std::sort(list.begin(), list.end());
        for (auto& e : list) nbr.push_back(e[0]), row_bit.push_back(2 * e[1] + e[2]);
        off.push_back((int)nbr.size());
    }
    expect("first valid row", &first, want_first);
    expect("entries", &entries, std::vector<int>{off[nodes]});
    expect("list offsets", g.off, off);
    expect("list neighbours", g.adj_nbr, nbr);
    expect("list rows", g.adj_row, row_bit);

    solver_component(g, anchor, nodes);
    std::vector<int> reach(nodes, 0), cid(nodes + 1, 0), cnode, shape;
    reach[anchor] = 1;
    for (int round = 0; round < nodes; ++round)
        for (int l = 0; l < R; ++l)
            if (rows[l].valid && (reach[rows[l].a] || reach[rows[l].b])) reach[rows[l].a] = reach[rows[l].b] = 1;
    for (int i = 0; i < nodes; ++i) {
        cid[i + 1] = cid[i] + reach[i];
        if (reach[i]) cnode.push_back(i);
    }
    int p2 = 1;
    while (p2 < cid[nodes]) p2 *= 2;
    shape = {cid[nodes], p2, cid[anchor]};
    const int got_shape[3] = {g.n, g.p2, g.anchor_c};
    expect("n, p2, anchor_c", got_shape, shape);
    expect("compact ids", g.cid, cid);
    expect("component nodes", g.cnode, cnode);
    for (int node : cnode) {
        std::vector<int> compact;
        for (int j = off[node]; j < off[node + 1]; ++j) compact.push_back(cid[nbr[j]]);
        expect("renumbered neighbours", g.adj_nbr + off[node], compact);
    }
    free(ws);
}

}  // namespace

int main() {
    const int settings[3][3] = {{1, 0, 0x00}, {SOLVER_THREADS, 1, 0xFF}, {64, 0, 0x55}};
    // 6 nodes: node 3 has no row, the pair (0, 1) twice (the rank tie goes to the row), an invalid row, both orientations
    const std::vector<Row> six = {{4, 2, 0}, {1, 0, 1}, {1, 2, 1}, {0, 1, 1}, {2, 4, 0}, {5, 4, 1}, {2, 0, 1}, {1, 0, 1}};
    const std::vector<Row> path = {{3, 4, 1}, {1, 0, 1}, {2, 3, 1}, {2, 1, 1}};  // 0 - 1 - 2 - 3 - 4: the most rounds from an end
    for (const auto& s : settings) {
        solver_host.lanes = s[0], solver_host.descending = s[1];
        for (int n : {0, 1, 255, 256, 257}) check_scan(n, s[2]);
        for (int n : {1, 2, 5}) check_tree(n, s[2]);  // p2 = 1, 2 and 8
        check_graph(six, 6, 3, s[2]);                 // an anchor no valid row touches: n = 1
        check_graph(six, 6, 4, s[2]);                 // two components: {4, 5} and {0, 1, 2}
        check_graph(six, 6, 0, s[2]);
        check_graph(path, 5, 0, s[2]);
        check_graph(path, 5, 4, s[2]);
    }
    if (failures) return 2;
    printf("problem_solver.h: scan, tree, lists and component equal the plain loops under 3 lane settings\n");
    return 0;
}
