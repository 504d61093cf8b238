// check_image_compare_host.cpp -- gsx_image_compare_host under the host sanitizers, as a program of its own (no Python, no device):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -Xarch_host -fno-sanitize-recover=undefined tools/check_image_compare_host.cpp \
//         3dgsconverter_amd/csrc/fidelity.hip -o /tmp/check_image_compare_host && /tmp/check_image_compare_host
//
// (-Xarch_host: the sanitizers instrument the host code alone; the kernel in the same file is compiled as always and never runs)
//
// Both images are heap blocks of exactly height * width * 3 bytes, so a byte read outside them is the sanitizer's finding; the
// nine words are compared with a direct evaluation of the definition: every window summed pixel by pixel in 64-bit
// integers, the two divisions and the product in plain double arithmetic.  Sizes: no window (7 x 7, 40 x 5), one window, one
// more column or row, the kernel's tile edge T + 6 ... T + 8, and 40 x 71; pairs: random, identical, black against white, an
// image against its complement.  Exit status 0: clean.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../3dgsconverter_amd/csrc/gsx_common.h"

namespace gsx {
static char g_error[512];
void set_error(const char *fmt, ...)   // (csrc/api.hip's, which this program does not link)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
int DevBuf::reserve(size_t) { return 1; }   // (the device entry point's buffer: never reached here)
void DevBuf::release() {}
}  // namespace gsx

static unsigned char *block(size_t bytes)
{
    unsigned char *p = static_cast<unsigned char *>(malloc(bytes ? bytes : 1));
    if (!p) abort();
    return p;
}

static void definition(const unsigned char *a, const unsigned char *b, int w, int h, int64_t *out)
{
    for (int k = 0; k < 9; ++k) out[k] = 0;
    for (int64_t i = 0; i < (int64_t)w * h * 3; ++i) out[i % 3] += ((int)a[i] - (int)b[i]) * ((int)a[i] - (int)b[i]);
    if (w < 8 || h < 8) return;
    out[3] = (int64_t)(w - 7) * (h - 7);
    for (int y = 0; y + 8 <= h; ++y)
        for (int x = 0; x + 8 <= w; ++x)
            for (int c = 0; c < 3; ++c) {
                int64_t sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                for (int dy = 0; dy < 8; ++dy)
                    for (int dx = 0; dx < 8; ++dx) {
                        const int64_t p = a[((int64_t)(y + dy) * w + x + dx) * 3 + c], q = b[((int64_t)(y + dy) * w + x + dx) * 3 + c];
                        sa += p, sb += q, saa += p * p, sbb += q * q, sab += p * q;
                    }
                const int64_t n1 = 2 * sa * sb + 26634, d1 = sa * sa + sb * sb + 26634;
                const int64_t n2 = 2 * (64 * sab - sa * sb) + 239708, d2 = (64 * saa - sa * sa) + (64 * sbb - sb * sb) + 239708;
                volatile double r1 = (double)n1 / (double)d1, r2 = (double)n2 / (double)d2;     // (volatile: each rounded on its own)
                volatile double prod = r1 * r2;
                out[4 + c] += (int64_t)floor(prod * 4294967296.0);
            }
}

static int check(int w, int h, int kind)
{
    const size_t bytes = (size_t)w * h * 3;
    unsigned char *a = block(bytes), *b = block(bytes);
    uint32_t s = 12345u + 977u * (uint32_t)w + 31u * (uint32_t)h + (uint32_t)kind;
    for (size_t i = 0; i < bytes; ++i) {
        s = s * 1664525u + 1013904223u;
        a[i] = (unsigned char)(s >> 24);
        s = s * 1664525u + 1013904223u;
        b[i] = kind == 0 ? (unsigned char)(s >> 24) : kind == 1 ? a[i] : kind == 2 ? 255 : (unsigned char)(255 - a[i]);
        if (kind == 2) a[i] = 0;
    }
    int64_t got[9], want[9];
    definition(a, b, w, h, want);
    int bad = 0;
    if (gsx_image_compare_host(a, b, w, h, got) != 0) {
        fprintf(stderr, "refused: %s\n", gsx::g_error);
        bad = 1;
    } else if (memcmp(got, want, sizeof(got)) != 0) {
        fprintf(stderr, "wrong words: %d x %d, pair %d\n", w, h, kind);
        bad = 1;
    }
    if (kind == 1 && !bad && (got[0] | got[1] | got[2] || got[4] != got[3] * 4294967296LL)) {
        fprintf(stderr, "identical images: %d x %d\n", w, h);
        bad = 1;
    }
    free(a);
    free(b);
    return bad;
}

int main()
{
    const int T = GSX_FIDELITY_TILE;
    const int sizes[][2] = {{7, 7}, {40, 5}, {8, 8}, {9, 8}, {8, 9}, {T + 6, T + 6}, {T + 7, T + 7}, {T + 8, T + 8}, {T + 8, T + 6}, {40, 71}, {1, 1}};
    int bad = 0, calls = 0;
    for (const auto &sz : sizes)
        for (int kind = 0; kind < 4; ++kind) {
            bad += check(sz[0], sz[1], kind);
            ++calls;
        }
    // a refusal reads nothing: sizes outside 1 ... 8192 on blocks of one pixel
    unsigned char *a = block(3), *b = block(3);
    int64_t words[9];
    if (gsx_image_compare_host(a, b, 0, 1, words) == 0) ++bad;
    if (gsx_image_compare_host(a, b, 1, 8193, words) == 0) ++bad;
    if (gsx_image_compare_host(a, nullptr, 1, 1, words) == 0) ++bad;
    free(a);
    free(b);
    printf("gsx_image_compare_host: %d image pairs, %d wrong\n", calls, bad);
    return bad != 0;
}
