// What the stand-alone host builds of the kernels' host/device functions (tools/*_host_main.cpp) share.
#pragma once

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../gtsfm_amd/csrc/common.h"

// the library's error sink: a refusal's reason goes to stderr
void gtsfm_set_error(const char* fmt, ...) {
    va_list args;
    va_start(args, fmt);
    vfprintf(stderr, fmt, args);
    va_end(args);
    fputc('\n', stderr);
}

namespace {

// n elements from f; *ok is cleared when they are not there
template <class T>
T* read_array(FILE* f, size_t n, bool* ok) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);  // exact size: the sanitizer sees every read past the end
    if (!p || (n && fread(p, sizeof(T), n, f) != n)) *ok = false;
    return p;
}

// a workspace: aligned to 256 bytes, every byte set to `fill`
void* filled(size_t bytes, int fill) {
    void* p = aligned_alloc(256, align_up(bytes ? bytes : 1, 256));
    if (p) memset(p, fill, align_up(bytes ? bytes : 1, 256));
    return p;
}

template <class T>
void fill_vector(std::vector<T>& v, size_t n, int fill) {
    v.assign(n + 1, T());  // one spare element: data() is never null
    memset(v.data(), fill, (n + 1) * sizeof(T));
    v.resize(n);
}

// the exit status for a pipeline's refusal; its reason is on stderr already (gtsfm_set_error)
int refused(int status) {
    fprintf(stderr, "refused (status %d)\n", status);
    return 3;
}

template <class T>
bool write_vector(FILE* f, const std::vector<T>& v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// `one` equals the elements of `all` from `at` on
template <class T>
bool same_slice(const std::vector<T>& all, size_t at, const std::vector<T>& one) {
    return one.empty() || memcmp(all.data() + at, one.data(), one.size() * sizeof(T)) == 0;
}

// n elements in an allocation of their exact size
template <class T>
T* copy_of(const T* from, size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, from, n * sizeof(T));
    return p;
}

}  // namespace
