// Stand-alone host build of the host side of the stage runner (gtsfm_amd/csrc/stage_runner.h), for running it on a CPU and under the host
// sanitizers; built like the other tools/*_host_main.cpp. It takes no argument.
//
// HostRunner's each, group, scan, fetch and zero run under its two settings -- ascending with one lane per group, descending with the
// stage's lane count -- on arrays allocated at their exact size, so a touch past the end is a sanitizer report:
//   each  : n in {0, 1, 255, 256, 257}: every index once, in the setting's order.
//   group : (groups, lanes) in {(1, 1), (3, 64), (0, 64)}: every (group, lane) once, in the setting's order, with the lane count it was told.
//   scan  : n in {0, 1, 4096, 4097} (SCAN_BLOCK is 4096) against a plain loop written here.
//   fetch, zero : exactly the bytes asked for, the neighbours on both sides untouched.
// Exit status 2: a difference, named on stderr.

#include "../gtsfm_amd/csrc/stage_runner.h"
#include "host_main_common.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, const HostRunner& run, long long n) {
    if (ok) return;
    fprintf(stderr, "%s differs at size %lld%s\n", what, n, run.descending ? ", descending with the device's lanes" : "");
    ++failures;
}

void check_each(HostRunner run, long long n) {
    int* hits = (int*)calloc(n ? n : 1, sizeof(int));
    std::vector<long long> order;
    const int status = run.each<struct probe_each_stage>(n, [&](long long i) { ++hits[i], order.push_back(i); });
    bool ok = status == GTSFM_OK && (long long)order.size() == n;
    for (long long k = 0; ok && k < n; ++k) ok = hits[k] == 1 && order[k] == (run.descending ? n - 1 - k : k);
    expect(ok, "each", run, n);
    free(hits);
}

template <int LANES>
void check_group(HostRunner run, long long groups) {
    const int want_lanes = run.device_lanes ? LANES : 1;
    const long long n = groups * want_lanes;
    int* hits = (int*)calloc(n ? n : 1, sizeof(int));
    std::vector<long long> order;
    bool told = true;
    run.group<struct probe_group_stage, 256, LANES>(groups, [&](long long group, int lane, int lanes) {
        told = told && lanes == want_lanes && lane >= 0 && lane < lanes;
        if (told) ++hits[group * lanes + lane], order.push_back(group * lanes + lane);
    });
    bool ok = told && (long long)order.size() == n;
    for (long long k = 0; ok && k < n; ++k) ok = hits[k] == 1 && order[k] == (run.descending ? n - 1 - k : k);
    expect(ok, "group", run, groups * 1000 + LANES);
    free(hits);
}

void check_scan(HostRunner run, long long n) {
    long long* val = (long long*)malloc((n + 1) * 8);
    std::vector<long long> want(n + 1, 0);
    memset(val, run.descending ? 0xFF : 0x00, (n + 1) * 8);
    for (long long i = 0; i < n; ++i) val[i] = (7 * i + 3) % 5, want[i + 1] = want[i] + val[i];
    run.scan(val, n);
    expect(memcmp(val, want.data(), (n + 1) * 8) == 0, "scan", run, n);
    free(val);
}

void check_fetch_and_zero(HostRunner run, size_t count) {
    std::vector<int> src(count + 2), dst(count + 2, 0x55555555), cleared(count + 2, 0x55555555);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (int)(i * 2654435761u);
    run.fetch(dst.data() + 1, src.data() + 1, count);
    run.zero(cleared.data() + 1, count * sizeof(int));
    bool ok = dst[0] == 0x55555555 && dst[count + 1] == 0x55555555 && cleared[0] == 0x55555555 && cleared[count + 1] == 0x55555555;
    for (size_t i = 1; ok && i <= count; ++i) ok = dst[i] == src[i] && cleared[i] == 0;
    expect(ok, "fetch / zero", run, (long long)count);
    int* exact = (int*)malloc(count ? count * sizeof(int) : 1);  // the whole of an exact-size allocation, and not a byte more
    run.fetch(exact, src.data(), count);
    run.zero(exact, count * sizeof(int));
    free(exact);
}

}  // namespace

int main() {
    for (const HostRunner run : {HostRunner{false, false}, HostRunner{true, true}}) {
        for (long long n : {0, 1, 255, 256, 257}) check_each(run, n);
        check_group<1>(run, 1), check_group<64>(run, 3), check_group<64>(run, 0);
        for (long long n : {0, 1, SCAN_BLOCK, SCAN_BLOCK + 1}) check_scan(run, n);
        for (size_t count : {0, 1, 7}) check_fetch_and_zero(run, count);
    }
    if (failures) return 2;
    printf("stage_runner.h: each, group, scan, fetch and zero equal the plain loops under both host settings\n");
    return 0;
}
