// dev_carve.h -- one buffer, several regions: the layout is written once and both sizes the buffer and places the regions.
// No HIP here: tools/check_dev_carve_host.cpp runs the same code on a heap block.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gsx {

// A layout is a callable that takes every region of a buffer in order through Carve::take.  It runs twice: on a null base it
// only measures (every take returns null), on the buffer's pointer it places.  The base itself must be aligned to the
// largest alignment the layout asks for (hipMalloc and hipHostMalloc return at least 256 bytes).
struct Carve {
    static constexpr size_t ALIGN = 256;
    char *base;
    size_t off = 0;
    explicit Carve(void *b) : base(static_cast<char *>(b)) {}
    // `count` elements of T at the next multiple of `align` (a power of two); a count of 0 is a valid empty region
    template <class T>
    T *take(size_t count, size_t align = ALIGN)
    {
        off = (off + align - 1) & ~(align - 1);
        T *r = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += sizeof(T) * count;
        return r;
    }
    size_t size() const { return off; }   // the end of the last region taken
};

template <class Layout>
size_t carve_measure(Layout &&layout)
{
    Carve m(nullptr);
    layout(m);
    return m.size();
}

// measure, reserve, place.  Buf: anything with `int reserve(size_t)` (0 = ok, grow-only) and a pointer `p` (DevBuf, PinnedBuf)
template <class Buf, class Layout>
int carve(Buf &buf, Layout &&layout)
{
    if (const int rc = buf.reserve(carve_measure(layout))) return rc;
    Carve a(buf.p);
    layout(a);
    return 0;
}

}  // namespace gsx
