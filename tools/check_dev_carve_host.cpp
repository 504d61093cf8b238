// check_dev_carve_host.cpp -- csrc/dev_carve.h under the host sanitizers, as a program of its own (no Python, no device, no HIP):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined
//       tools/check_dev_carve_host.cpp -o /tmp/check_dev_carve_host && /tmp/check_dev_carve_host
//
// (through hipcc: the same flags behind -Xarch_host, as for tools/check_rows_remap_host.cpp)
//
// The layouts below mirror the ones the library carves its context buffers with (csrc/*.hip: morton_order_dev,
// launch_assign_mfma_t, alloc_table, kmeans1d_dev, the radix-sort sites, gsx_rgb_from_sh_list, voxel_clusters_dev, the slab
// step's small block), at sizes 0, 1, 63, 64, 65 and 4097.  For each: the measured size is the end of the last region, measuring
// does not depend on the base, regions do not overlap, every region meets its alignment, a region of count 0 is a valid empty
// one, and every region is filled through its pointer inside a heap block of EXACTLY the measured size -- an overrun is the
// sanitizer's finding, an overlap shows when the fill is read back.  Exit status 0: clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../3dgsconverter_amd/csrc/dev_carve.h"

using gsx::Carve;

struct Region {
    char *p;
    size_t bytes, align;
};

// Carve::take, with a record of what was taken
struct Rec {
    Carve &a;
    std::vector<Region> &out;
    template <class T>
    T *take(size_t count, size_t align = Carve::ALIGN)
    {
        T *r = a.take<T>(count, align);
        out.push_back({reinterpret_cast<char *>(r), sizeof(T) * count, align});
        return r;
    }
};

using Layout = std::function<void(Rec &)>;

static int g_failures = 0;

#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            ++g_failures;                  \
            fprintf(stderr, "FAIL %s: ", name); \
            fprintf(stderr, __VA_ARGS__);  \
            fprintf(stderr, "\n");         \
        }                                  \
    } while (0)

static size_t run(const Layout &layout, void *base, std::vector<Region> *regions)
{
    Carve a(base);
    regions->clear();
    Rec r{a, *regions};
    layout(r);
    return a.size();
}

static void check(const char *name, const Layout &layout)
{
    std::vector<Region> m, p1, p2;
    const size_t size = run(layout, nullptr, &m);
    EXPECT(!m.empty(), "no region");
    for (const Region &r : m) EXPECT(r.p == nullptr, "the measuring pass returned a pointer");
    // two blocks of exactly the measured size at different addresses (the second behind a spacer, so that the bases differ
    // in more than their low bits)
    void *b1 = nullptr, *spacer = nullptr, *b2 = nullptr;
    if (posix_memalign(&b1, Carve::ALIGN, size ? size : 1) || posix_memalign(&spacer, Carve::ALIGN, 4096 + 256) ||
        posix_memalign(&b2, Carve::ALIGN, size ? size : 1))
        abort();
    EXPECT(run(layout, b1, &p1) == size, "placing on a base measured another size than the null base");
    EXPECT(run(layout, b2, &p2) == size, "placing on a second base measured another size");
    EXPECT(p1.size() == m.size() && p2.size() == m.size(), "the passes took different numbers of regions");
    size_t end = 0;
    for (size_t i = 0; i < p1.size() && i < p2.size(); ++i) {
        const Region &r = p1[i];
        EXPECT(r.p != nullptr, "region %zu is null in the placing pass", i);
        const size_t off = (size_t)(r.p - static_cast<char *>(b1));
        EXPECT(off == (size_t)(p2[i].p - static_cast<char *>(b2)), "region %zu sits at another offset on another base", i);
        EXPECT(r.bytes == m[i].bytes && r.align == m[i].align, "region %zu differs between the passes", i);
        EXPECT(off >= end, "region %zu (offset %zu) overlaps the one before it (end %zu)", i, off, end);
        EXPECT(off % r.align == 0 && reinterpret_cast<uintptr_t>(r.p) % r.align == 0, "region %zu (offset %zu) misses its alignment %zu", i, off,
               r.align);
        EXPECT(off + r.bytes <= size, "region %zu ends at %zu, behind the measured size %zu", i, off + r.bytes, size);   // (also for count 0)
        end = off + r.bytes;
    }
    EXPECT(end == size, "the measured size %zu is not the last region's end %zu", size, end);
    // fill every region through its pointer, then read every fill back
    if (g_failures == 0) {
        for (size_t i = 0; i < p1.size(); ++i) memset(p1[i].p, (int)(i + 1), p1[i].bytes);
        for (size_t i = 0; i < p1.size(); ++i)
            for (size_t b = 0; b < p1[i].bytes; ++b)
                if ((unsigned char)p1[i].p[b] != (unsigned char)(i + 1)) {
                    EXPECT(false, "byte %zu of region %zu was overwritten by another region", b, i);
                    break;
                }
    }
    free(b1);
    free(spacer);
    free(b2);
}

// ---- the layouts (the element types stand in for the library's: same size, same alignment requests)
struct U32x4 {
    uint32_t w[4];
};
struct Block32 {   // VoxelFrame, CcOut
    uint32_t w[8];
};

static Layout morton(size_t n, size_t temp_bytes)   // cply.hip: morton_order_dev
{
    return [=](Rec &a) {
        const size_t per = n + 64;
        for (int i = 0; i < 4; ++i) a.take<uint32_t>(per);   // pos / seg, ping-pong
        a.take<uint32_t>(6 * per);                           // boxes
        a.take<uint64_t>(per), a.take<uint64_t>(per);        // keys
        a.take<uint32_t>(per), a.take<uint32_t>(per);        // values
        a.take<uint8_t>(per);                                // flags
        a.take<uint32_t>(64);                                // counts
        a.take<char>(temp_bytes);
    };
}

static Layout kmeans_operands(int d, int k, size_t nprob, size_t n_total)   // kmeans.hip: launch_assign_mfma_t
{
    return [=](Rec &a) {
        const size_t ns = (size_t)((d + 3 + 15) / 16), ktiles = (size_t)((k + 31) / 32);
        a.take<U32x4>(ktiles * ns * 2 * 64 * nprob);
        a.take<uint32_t>(32 * nprob, 16);   // meta
        a.take<uint32_t>(n_total, 4);       // list
        a.take<uint32_t>((size_t)k * nprob, 4), a.take<uint32_t>((size_t)k * nprob, 4);   // starts, cursor
        a.take<uint32_t>(16, 4);
    };
}

static Layout kmeans_sums(int d, int k, size_t nprob)   // kmeans.hip: kmeans_lloyd_dev, lloyd_batch_mfma
{
    return [=](Rec &a) {
        a.take<double>((size_t)k * d * nprob);
        a.take<uint32_t>((size_t)k * nprob, 4);
        a.take<int64_t>(nprob + 1, 64);
        a.take<char>(64, 1);
    };
}

static Layout voxel_table(size_t items, bool wide, size_t out_bytes)   // density.hip: alloc_table
{
    return [=](Rec &a) {
        size_t tsize = 1024;
        while (tsize < 2 * items) tsize <<= 1;
        a.take<uint64_t>(tsize);
        a.take<uint32_t>(tsize, 4);
        if (wide) a.take<uint32_t>(tsize, 4);
        a.take<char>(out_bytes, 16);
        a.take<char>(64, 1);
    };
}

static Layout voxel_clusters(size_t m)   // density.hip: voxel_clusters_dev
{
    return [=](Rec &a) {
        a.take<int64_t>(3);
        a.take<Block32>(1, 64);
        a.take<int64_t>(3 * m);
        a.take<uint8_t>(m);
        a.take<uint8_t>(16, 1);
    };
}

static Layout kmeans1d(size_t n, size_t temp_bytes)   // kmeans1d.hip: kmeans1d_dev
{
    return [=](Rec &a) {
        const size_t ntiles = (n + 2047) / 2048;
        a.take<uint32_t>(n), a.take<uint32_t>(n), a.take<float>(n);
        a.take<double>(n), a.take<double>(n);
        a.take<double>(2 * (ntiles + 2));
        a.take<uint32_t>(16);
        a.take<double>(8, 8);
        a.take<float>(2 * 1024);
        a.take<char>(temp_bytes);
    };
}

static Layout sort_pairs(size_t n, size_t temp_bytes)   // sog.hip: lexsort3_dev, sog_table.hip: gsx_sog_order_dev
{
    return [=](Rec &a) {
        a.take<uint32_t>(n);
        for (int i = 0; i < 3; ++i) a.take<uint32_t>(n, 4);
        a.take<char>(temp_bytes);
    };
}

static Layout rgb_list(size_t n, size_t cap)   // api.hip: gsx_rgb_from_sh_list
{
    return [=](Rec &a) {
        a.take<uint8_t>(n);
        a.take<uint32_t>(4, 16);
        a.take<uint32_t>(cap, 4);
        a.take<uint8_t>(16, 1);
    };
}

static Layout slab_small()   // dist_slab.hip: slab_step_body
{
    return [](Rec &a) {
        a.take<uint32_t>(32);
        a.take<uint32_t>(2, 8), a.take<uint32_t>(2, 8);
        a.take<float>(4, 16);
    };
}

int main()
{
    const size_t sizes[] = {0, 1, 63, 64, 65, 4097};
    char label[128];
    for (const size_t n : sizes) {
        snprintf(label, sizeof(label), "morton n=%zu", n);
        check(label, morton(n, 1234 + 16 * n));
        for (const int d : {9, 24, 45})
            for (const size_t nprob : {(size_t)1, (size_t)3})
                for (const int k : {64, 100}) {
                    snprintf(label, sizeof(label), "kmeans operands D=%d K=%d nprob=%zu n=%zu", d, k, nprob, n);
                    check(label, kmeans_operands(d, k, nprob, n * nprob));
                    snprintf(label, sizeof(label), "kmeans sums D=%d K=%d nprob=%zu", d, k, nprob);
                    check(label, kmeans_sums(d, k, nprob));
                }
        for (const bool wide : {false, true})
            for (const size_t out_bytes : {(size_t)64, 16 * (n ? n : 1) + 64}) {
                snprintf(label, sizeof(label), "voxel table %s items=%zu out=%zu", wide ? "wide" : "narrow", n, out_bytes);
                check(label, voxel_table(n, wide, out_bytes));
            }
        snprintf(label, sizeof(label), "voxel clusters m=%zu", n);
        check(label, voxel_clusters(n));
        snprintf(label, sizeof(label), "kmeans1d n=%zu", n);
        check(label, kmeans1d(n, 777 + n));
        snprintf(label, sizeof(label), "sort pairs n=%zu", n);
        check(label, sort_pairs(n, 1 + 8 * n));
        for (const size_t cap : {(size_t)0, n}) {
            snprintf(label, sizeof(label), "rgb list n=%zu cap=%zu", n, cap);
            check(label, rgb_list(n, cap));
        }
    }
    check("slab small", slab_small());
    // the helper that does measure + reserve + place in one call, on a stand-in buffer: grow-only, and the pointers of the
    // second pass lie inside the block it reserved
    struct HeapBuf {
        void *p = nullptr;
        size_t cap = 0;
        int reserves = 0;
        int reserve(size_t bytes)
        {
            if (bytes <= cap) return 0;
            free(p);
            if (posix_memalign(&p, Carve::ALIGN, bytes)) return 1;
            cap = bytes;
            ++reserves;
            return 0;
        }
        ~HeapBuf() { free(p); }
    } buf;
    {
        const char *name = "carve()";
        for (const size_t n : {(size_t)65, (size_t)4097, (size_t)65}) {
            uint32_t *a1 = nullptr;
            uint8_t *a2 = nullptr;
            const int rc = gsx::carve(buf, [&](Carve &a) { a1 = a.take<uint32_t>(n), a2 = a.take<uint8_t>(n, 16); });
            EXPECT(rc == 0 && a1 && a2, "carve() failed");
            if (a1 && a2) {
                memset(a1, 1, 4 * n);
                memset(a2, 2, n);
                EXPECT(reinterpret_cast<char *>(a2) + n <= static_cast<char *>(buf.p) + buf.cap, "carve() placed a region behind its buffer");
            }
        }
        EXPECT(buf.reserves == 2, "carve() reserved %d times for sizes 65, 4097, 65 (expected 2: grow-only)", buf.reserves);
    }
    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("check_dev_carve_host: all layouts clean\n");
    return 0;
}
