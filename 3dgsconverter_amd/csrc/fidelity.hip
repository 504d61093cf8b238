// fidelity.hip -- two rendered images compared in integers (--fidelity): per-channel squared error and a box-window SSIM in 32.32
// fixed point.  No counterpart in the reference; the definition is tests/fidelity_numpy.py, and the nine words here
// are that file's on every run: every addend is an integer, so neither the tiling nor the order the workgroups arrive in shows.
//
//   gsx_image_compare_dev    one launch over tiles of FID_TILE x FID_TILE pixels (and window origins)
//   gsx_image_compare_host   the same from the same per-window function, serial, for the host tests
//
// A workgroup of 256 lanes owns the pixels [x0, x0 + T) x [y0, y0 + T) for the squared error and the windows whose top-left
// corner lies there.  (a) both images' (T + 7) x (T + 7) x 3 bytes come into LDS, a byte per lane and round (rows of 3 w bytes have
// no alignment to widen on), bytes outside the image as 0 -- no window that exists reads them; the squared differences of the
// owned pixels are summed on the way.  Per channel: (b) the horizontal pass, the five sums Sa, Sb, Saa, Sbb, Sab over 8 pixels for
// every staged row and window column, u32 in LDS; (c) the vertical pass over 8 of those rows, one window per lane and round, then
// q (fid_q) for the windows that exist.  (d) three u64 error sums and three i64 q sums per lane -> wave shuffles -> LDS -> one 64-bit
// integer atomicAdd per workgroup and quantity.  LDS: 2 x 4564 + 5 x 39 x 32 x 4 = 34088 bytes, four workgroups per CU.
//
// fid_q is the one place with floating point: four integers below 2^31 converted exactly, two correctly rounded divisions, one
// product, an exact scaling by 2^32 and floor.  The build's -ffp-contract=off and the pragma below keep the host from fusing
// anything; the device goes through __ddiv_rn / __dmul_rn.
#include <cmath>

#include "gsx_common.h"

namespace gsx {

constexpr int FID_TILE = GSX_FIDELITY_TILE;
constexpr int FID_WIN = 8;                                   // the window's side; N = 64 pixels
constexpr int FID_SPAN = FID_TILE + FID_WIN - 1;             // staged pixels per side
constexpr int FID_ROW_BYTES = FID_SPAN * 3;
constexpr int FID_STAGE_BYTES = (FID_SPAN * FID_ROW_BYTES + 3) / 4 * 4;
constexpr int FID_H = FID_SPAN * FID_TILE;                   // horizontal sums of one quantity
constexpr int FID_THREADS = 256;
constexpr int FID_C1 = 26634, FID_C2 = 239708;               // round(N^2 (0.01 * 255)^2), round(N^2 (0.03 * 255)^2)

// the fixed-point SSIM of one window from its five sums.  Every integer expression stays below 2^31 in magnitude: 2 Sa Sb + c1 and
// Sa^2 + Sb^2 + c1 <= 2 * 16320^2 + c1 = 532 711 434; N Sab <= 266 342 400.
__host__ __device__ inline long long fid_q(int sa, int sb, int saa, int sbb, int sab)
{
#pragma clang fp contract(off)
    const int ab = sa * sb, a2 = sa * sa, b2 = sb * sb;
    const int n1 = 2 * ab + FID_C1, d1 = a2 + b2 + FID_C1;
    const int n2 = 2 * (64 * sab - ab) + FID_C2, d2 = (64 * saa - a2) + (64 * sbb - b2) + FID_C2;
#ifdef __HIP_DEVICE_COMPILE__
    const double r1 = __ddiv_rn((double)n1, (double)d1), r2 = __ddiv_rn((double)n2, (double)d2);
    const double v = __dmul_rn(__dmul_rn(r1, r2), 4294967296.0);
#else
    const double r1 = (double)n1 / (double)d1, r2 = (double)n2 / (double)d2;
    const double p = r1 * r2;
    const double v = p * 4294967296.0;
#endif
    return (long long)floor(v);
}

__device__ inline unsigned long long fid_wave_sum(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);     // (integer adds: the same whatever their order)
    return v;
}

__global__ __launch_bounds__(FID_THREADS) void image_compare_kernel(const unsigned char *__restrict__ A, const unsigned char *__restrict__ B,
                                                                    int width, int height, int tiles_x, unsigned long long *__restrict__ out)
{
    __shared__ unsigned char s_a[FID_STAGE_BYTES], s_b[FID_STAGE_BYTES];
    __shared__ unsigned s_h[5][FID_H];
    __shared__ unsigned long long s_part[FID_THREADS / WAVE][6];
    const int t = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * FID_TILE, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * FID_TILE;
    const int64_t row_bytes = (int64_t)width * 3;

    // (a) stage, and the squared error of the owned pixels
    unsigned e0 = 0, e1 = 0, e2 = 0;                      // <= 36 bytes per lane, 65025 each
    for (int i = t; i < FID_SPAN * FID_ROW_BYTES; i += FID_THREADS) {
        const int r = i / FID_ROW_BYTES, b = i - r * FID_ROW_BYTES;
        const int gy = y0 + r;
        const int64_t gb = (int64_t)x0 * 3 + b;
        unsigned va = 0, vb = 0;
        if (gy < height && gb < row_bytes) {
            const int64_t at = (int64_t)gy * row_bytes + gb;
            va = A[at];
            vb = B[at];
            if (r < FID_TILE && b < FID_TILE * 3) {
                const int df = (int)va - (int)vb;
                const unsigned sq = (unsigned)(df * df);
                const int c = b % 3;
                e0 += c == 0 ? sq : 0u;
                e1 += c == 1 ? sq : 0u;
                e2 += c == 2 ? sq : 0u;
            }
        }
        s_a[i] = (unsigned char)va;
        s_b[i] = (unsigned char)vb;
    }
    __syncthreads();

    long long q[3] = {0, 0, 0};
    const int wx_end = width - (FID_WIN - 1) - x0, wy_end = height - (FID_WIN - 1) - y0;   // window origins of this tile that exist: below these
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // (b) horizontal: staged row r, window column x
        for (int i = t; i < FID_H; i += FID_THREADS) {
            const int r = i / FID_TILE, x = i % FID_TILE;
            const int at = r * FID_ROW_BYTES + x * 3 + c;
            unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
            for (int k = 0; k < FID_WIN; ++k) {
                const unsigned a = s_a[at + 3 * k], b = s_b[at + 3 * k];
                sa += a;
                sb += b;
                saa += a * a;
                sbb += b * b;
                sab += a * b;
            }
            s_h[0][i] = sa;
            s_h[1][i] = sb;
            s_h[2][i] = saa;
            s_h[3][i] = sbb;
            s_h[4][i] = sab;
        }
        __syncthreads();
        // (c) vertical: window (x, y) of the tile
        for (int i = t; i < FID_TILE * FID_TILE; i += FID_THREADS) {
            const int y = i / FID_TILE, x = i % FID_TILE;
            if (x < wx_end && y < wy_end) {
                unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
                for (int k = 0; k < FID_WIN; ++k) {
                    const int at = (y + k) * FID_TILE + x;
                    sa += s_h[0][at];
                    sb += s_h[1][at];
                    saa += s_h[2][at];
                    sbb += s_h[3][at];
                    sab += s_h[4][at];
                }
                q[c] += fid_q((int)sa, (int)sb, (int)saa, (int)sbb, (int)sab);
            }
        }
        __syncthreads();
    }

    // (d) lane -> wave -> workgroup -> the six global words (two's complement: the signed sums add as unsigned words)
    unsigned long long v[6] = {e0, e1, e2, (unsigned long long)q[0], (unsigned long long)q[1], (unsigned long long)q[2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = fid_wave_sum(v[k]);
    if ((t & (WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_part[t / WAVE][k] = v[k];
    }
    __syncthreads();
    if (t < 6) {
        unsigned long long s = 0;
        for (int w = 0; w < FID_THREADS / WAVE; ++w) s += s_part[w][t];
        if (s) atomicAdd(&out[t], s);
    }
}

static int fid_check(const void *a, const void *b, int32_t width, int32_t height, const int64_t *out_words, const char *who)
{
    if (!a || !b || !out_words) GSX_FAIL("%s: null argument", who);
    if (width < 1 || width > GSX_FIDELITY_MAX_SIDE || height < 1 || height > GSX_FIDELITY_MAX_SIDE)
        GSX_FAIL("%s: an image of %d x %d (1 ... %d per side)", who, width, height, GSX_FIDELITY_MAX_SIDE);
    return 0;
}

static inline int64_t fid_windows(int32_t width, int32_t height)
{
    return width >= FID_WIN && height >= FID_WIN ? (int64_t)(height - (FID_WIN - 1)) * (width - (FID_WIN - 1)) : 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" int gsx_image_compare_dev(gsx_ctx *c, const void *a_dev, const void *b_dev, int32_t width, int32_t height, int64_t *out_words,
                                     float *stage_ms)
{
    const char *who = "gsx_image_compare_dev";
    if (!c) GSX_FAIL("%s: null argument", who);
    GSX_CHECK(fid_check(a_dev, b_dev, width, height, out_words, who));
    GSX_HIP(hipSetDevice(c->device));
    GSX_CHECK(c->work.reserve(6 * sizeof(unsigned long long)));
    unsigned long long *sums = c->work.as<unsigned long long>();
    const int tiles_x = (width + FID_TILE - 1) / FID_TILE, tiles_y = (height + FID_TILE - 1) / FID_TILE;   // <= 256 x 256
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard()
        {
            for (int k = 0; k < 2; ++k)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } guard{ev};
    GSX_HIP(hipMemsetAsync(sums, 0, 6 * sizeof(unsigned long long), c->stream));
    if (stage_ms) {
        GSX_HIP(hipEventCreate(&ev[0]));
        GSX_HIP(hipEventCreate(&ev[1]));
        GSX_HIP(hipEventRecord(ev[0], c->stream));
    }
    hipLaunchKernelGGL(image_compare_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(FID_THREADS), 0, c->stream,
                       static_cast<const unsigned char *>(a_dev), static_cast<const unsigned char *>(b_dev), (int)width, (int)height, tiles_x, sums);
    GSX_HIP(hipGetLastError());
    if (stage_ms) GSX_HIP(hipEventRecord(ev[1], c->stream));
    unsigned long long host[6] = {0, 0, 0, 0, 0, 0};
    GSX_HIP(hipMemcpyAsync(host, sums, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if (stage_ms) {
        float ms = 0.0f;
        GSX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *stage_ms += ms;
    }
    for (int k = 0; k < GSX_FIDELITY_WORDS; ++k) out_words[k] = 0;
    for (int k = 0; k < 3; ++k) {
        out_words[k] = (int64_t)host[k];
        out_words[4 + k] = (int64_t)host[3 + k];
    }
    out_words[3] = fid_windows(width, height);
    return 0;
}

extern "C" int gsx_image_compare_host(const void *a, const void *b, int32_t width, int32_t height, int64_t *out_words)
{
    GSX_CHECK(fid_check(a, b, width, height, out_words, "gsx_image_compare_host"));
    const unsigned char *A = static_cast<const unsigned char *>(a), *B = static_cast<const unsigned char *>(b);
    const size_t row_bytes = (size_t)width * 3;
    for (int k = 0; k < GSX_FIDELITY_WORDS; ++k) out_words[k] = 0;
    for (size_t i = 0; i < row_bytes * (size_t)height; ++i) {
        const int df = (int)A[i] - (int)B[i];
        out_words[i % 3] += df * df;
    }
    out_words[3] = fid_windows(width, height);
    if (!out_words[3]) return 0;
    // column sums of the five quantities over the rows y ... y + 7, per channel byte: a row enters, the row above the window leaves
    // (unsigned arithmetic: the differences are exact); a window's sums are those of its 8 columns
    std::vector<unsigned> col(5 * row_bytes, 0u);
    unsigned *ca = col.data(), *cb = ca + row_bytes, *caa = cb + row_bytes, *cbb = caa + row_bytes, *cab = cbb + row_bytes;
    for (int y = 0; y < height; ++y) {
        const unsigned char *ra = A + (size_t)y * row_bytes, *rb = B + (size_t)y * row_bytes;
        for (size_t i = 0; i < row_bytes; ++i) {
            const unsigned p = ra[i], r = rb[i];
            ca[i] += p;
            cb[i] += r;
            caa[i] += p * p;
            cbb[i] += r * r;
            cab[i] += p * r;
        }
        if (y >= FID_WIN) {
            const unsigned char *oa = A + (size_t)(y - FID_WIN) * row_bytes, *ob = B + (size_t)(y - FID_WIN) * row_bytes;
            for (size_t i = 0; i < row_bytes; ++i) {
                const unsigned p = oa[i], r = ob[i];
                ca[i] -= p;
                cb[i] -= r;
                caa[i] -= p * p;
                cbb[i] -= r * r;
                cab[i] -= p * r;
            }
        }
        if (y < FID_WIN - 1) continue;
        for (int x = 0; x + FID_WIN <= width; ++x)
            for (int c = 0; c < 3; ++c) {
                unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                for (int k = 0; k < FID_WIN; ++k) {
                    const size_t i = (size_t)(x + k) * 3 + c;
                    sa += ca[i];
                    sb += cb[i];
                    saa += caa[i];
                    sbb += cbb[i];
                    sab += cab[i];
                }
                out_words[4 + c] += fid_q((int)sa, (int)sb, (int)saa, (int)sbb, (int)sab);
            }
    }
    return 0;
}
