// check_rows_remap_host.cpp -- gsx_rows_remap_host under the host sanitizers, as a program of its own (no Python, no device):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -Xarch_host -fno-sanitize-recover=undefined tools/check_rows_remap_host.cpp 3dgsconverter_amd/csrc/rows_remap.hip \
//         -pthread -o /tmp/check_rows_remap_host && /tmp/check_rows_remap_host
//
// (-Xarch_host: the sanitizers instrument the host code alone; the kernel in the same file is compiled as always and never runs)
//
// Source and destination are heap blocks of exactly the bytes the contract allows the call to touch (the rows; the destination
// with guard rows around the written range), so a byte read or written outside them is the sanitizer's finding; the result is
// compared with a byte loop over the same runs.  Shapes: n in (0, 1, 129, 5000), several first bytes and row offsets, a widening
// (107 -> 251 bytes), a narrowing with dropped fields (300 -> 248) and the whole-row copy.  Exit status 0: clean.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/gsx_hip.h"

namespace gsx {
static char g_error[512];
void set_error(const char *fmt, ...)   // (csrc/api.hip's, which this program does not link)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace gsx

struct Run {
    int32_t src, dst, len;
};

// a 16-byte aligned heap block of exactly `bytes` bytes (at least one)
static unsigned char *block(size_t bytes)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1) != 0) abort();
    return static_cast<unsigned char *>(p);
}

// runs of 1 ... 13 bytes at any offset, a third of them zero fill, source bytes skipped in between (dropped fields); `whole`: the
// one run of a source in the destination's own layout
static std::vector<Run> make_runs(int si, int so, bool whole)
{
    std::vector<Run> runs;
    if (whole) return {{0, 0, so}};
    int s = 1, d = 0;
    while (d < so) {
        const int len = std::min(so - d, 1 + (d * 7 + 3) % 13);
        const bool zero = (d / 5) % 3 == 1 || s + len > si;
        runs.push_back({zero ? -1 : s, d, len});
        if (!zero) s += len + (d % 2);
        d += len;
    }
    return runs;
}

static int check(int si, int so, int64_t n, int64_t row0, int64_t rows, int src_first, int dst_first, bool whole)
{
    const std::vector<Run> runs = make_runs(si, so, whole);
    if (runs.size() > 128) return 0;
    // 16-byte aligned bases; the blocks end with the last row (no slack: the host twin reads and writes rows only)
    const size_t sbytes = (size_t)src_first + (size_t)n * si, dbytes = (size_t)dst_first + (size_t)rows * so;
    unsigned char *src = block(sbytes), *dst = block(dbytes);
    std::vector<unsigned char> want(dbytes, 0xA5);
    for (size_t i = 0; i < sbytes; ++i) src[i] = (unsigned char)(i * 131 + 7);
    memset(dst, 0xA5, dbytes);
    for (int64_t r = 0; r < n; ++r)
        for (const Run &u : runs)
            for (int i = 0; i < u.len; ++i)
                want[dst_first + (row0 + r) * so + u.dst + i] = u.src < 0 ? 0 : src[src_first + r * si + u.src + i];
    const int rc = gsx_rows_remap_host(src, src_first, si, n, &runs[0].src, (int)runs.size(), dst, dst_first, so, row0, rows);
    int bad = 0;
    if (rc != 0) {
        fprintf(stderr, "refused: %s\n", gsx::g_error);
        bad = 1;
    } else if (memcmp(dst, want.data(), dbytes) != 0) {
        fprintf(stderr, "wrong bytes: %d -> %d bytes, %lld rows at row %lld of %lld\n", si, so, (long long)n, (long long)row0, (long long)rows);
        bad = 1;
    }
    free(src);
    free(dst);
    return bad;
}

int main()
{
    int bad = 0, calls = 0;
    const int shapes[][2] = {{107, 251}, {300, 248}, {71, 248}, {251, 251}, {1, 512}, {512, 1}};
    const int64_t sizes[] = {0, 1, 129, 5000};
    for (const auto &sh : shapes)
        for (int64_t n : sizes)
            for (int64_t row0 : {(int64_t)0, (int64_t)3})
                for (int first : {0, 5, 15}) {
                    bad += check(sh[0], sh[1], n, row0, n + row0 + 2, first, 15 - first, false);
                    if (sh[0] == sh[1]) bad += check(sh[0], sh[1], n, row0, n + row0 + 2, first, 15 - first, true);
                    ++calls;
                }
    // a refusal writes nothing and reads nothing: a run that leaves the source row, on blocks of one row each
    unsigned char *a = block(8), *b = block(8);
    const int32_t past[3] = {5, 0, 8};
    if (gsx_rows_remap_host(a, 0, 8, 1, past, 1, b, 0, 8, 0, 1) == 0) ++bad;
    free(a);
    free(b);
    printf("gsx_rows_remap_host: %d shapes, %d wrong\n", calls, bad);
    return bad != 0;
}
