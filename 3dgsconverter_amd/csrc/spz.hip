// spz.hip -- numeric core of the SPZ v3 writer: the whole packed body of a `.spz` file from the raw rows of a splat table.
//
// Replaces, in gsconverter/formats/spz.py:
//   write, SH detection      :60-77    `np.any(data[f] != 0)` per strided f_rest column   -> rest_scan_kernel (rest_scan.h)
//   _pack_v3                 :111-170  positions, alpha, colours, scales, SH              -> spz_pack_kernel
//   _pack_rot_v3             :298-343  smallest-three quaternion words (a per-splat loop) -> spz_pack_kernel
//
// The body is six sections, each a contiguous span of the output:
//   positions 9n @ 0 | alpha n @ 9n | colours 3n @ 10n | scales 3n @ 13n | rotations 4n @ 16n | SH 3*sh_dim*n @ 20n
// One workgroup owns a tile of consecutive rows: the tile's raw bytes are staged in LDS with 16-byte loads (any row size up
// to 512 bytes, fields at any byte offset: a field is assembled from two LDS words), every thread packs one row into an LDS
// image of the tile's six section slices, and the workgroup then writes each slice -- 9, 1, 3, 3, 4 and 3*sh_dim bytes per
// row -- as one contiguous span with 16-byte stores (byte stores only at the two unaligned ends of a span).
//
// Every float32 operation is numpy's, in numpy's order (the library is built with -ffp-contract=off), with numpy's casts as
// they behave on x86: float32 -> int32 of NaN, +-inf or |v| >= 2^31 gives INT_MIN; float32 -> uint8 of NaN gives 0.  Two
// results are left to the host, listed per row in `list_dev`:
//   kind 0  the alpha byte when the float64 exp bracket of numpy's float32 SIMD exp straddles a byte boundary, or for NaN
//   kind 1  the rotation word when a component other than the largest is NaN (numpy's float32 -> uint32 cast of a NaN
//           depends on where in its array the value sits: vector lanes and scalar remainder differ)
#include "gsx_common.h"
#include "sog_math.h"
#include "row_tile.h"
#include "rest_scan.h"

namespace gsx {

__host__ __device__ constexpr int spz_sh_dim(int degree) { return degree == 1 ? 3 : degree == 2 ? 8 : degree == 3 ? 15 : 0; }
__host__ __device__ constexpr int spz_row_out_bytes(int sh_dim) { return 20 + 3 * sh_dim; }

// numpy's float32 -> int32 cast on x86 (cvttss2si): NaN, +-inf and values outside [-2^31, 2^31) give INT_MIN
__device__ __forceinline__ int spz_f32_to_i32(float t)
{
    return (t == t && t >= -2147483648.0f && t < 2147483648.0f) ? (int)t : (int)0x80000000u;
}

// quant_sh (spz.py:162-170) for one value: round(v * 128 + 128) -> int32, (q + bs/2) // bs * bs, clip 0..255; bs = 1 << shift
__device__ __forceinline__ unsigned spz_sh_byte(float v, int shift)
{
    const float t = rintf(__fadd_rn(__fmul_rn(v, 128.0f), 128.0f));
    const int q = spz_f32_to_i32(t);
    const int f = ((q + (1 << (shift - 1))) >> shift) * (1 << shift);   // floor division: arithmetic shift (no overflow: |q| < 2^31 - 8)
    return (unsigned)min(max(f, 0), 255);
}

// spz.py:298-343 for one splat (w, x, y, z = rot_0..3).  *host = a non-largest component is NaN (see the file header)
__device__ __forceinline__ unsigned spz_rot_word(float w, float x, float y, float z, bool *host)
{
    float s = __fmul_rn(w, w);
    s = __fadd_rn(s, __fmul_rn(x, x));
    s = __fadd_rn(s, __fmul_rn(y, y));
    s = __fadd_rn(s, __fmul_rn(z, z));
    s = __fadd_rn(s, (float)1e-9);                    // + 1e-9: a weak Python scalar, rounded to float32 first
    const float nrm = __builtin_sqrtf(s);             // correctly rounded (see sog_math.h: sog_quat_pack)
    float r[4] = {__fdiv_rn(x, nrm), __fdiv_rn(y, nrm), __fdiv_rn(z, nrm), __fdiv_rn(w, nrm)};   // X, Y, Z, W
    int mi = 0;
    float ma = -1.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {                     // np.argmax(np.abs(R)): the first maximum, or the first NaN
        const float a = fabsf(r[c]);
        if (a != a) {
            if (ma == ma) {
                mi = c;
                ma = a;
            }
        } else if (a > ma) {
            mi = c;
            ma = a;
        }
    }
    const bool neg = r[mi] < 0.0f;
    const float scale = (float)(511.0 / 0.707106781186547524401);
    unsigned word = (unsigned)mi << 30;
    bool nan = false;
    int slot = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c == mi) continue;
        const float v = r[c];
        nan |= v != v;
        const unsigned negbit = (v < 0.0f) != neg ? 1u : 0u;
        const float m = fminf(fmaxf(__fadd_rn(__fmul_rn(fabsf(v), scale), 0.5f), 0.0f), 511.0f);
        const unsigned mag = v == v ? (unsigned)m : 0u;
        word |= ((negbit << 9) | mag) << ((2 - slot) * 10);
        ++slot;
    }
    *host = nan;
    return word;
}

// rows -> the six section slices of every tile
__global__ void spz_pack_kernel(const uint4 *__restrict__ rows, SpzLayoutDev L, int64_t n, int sh_dim, unsigned char *__restrict__ out,
                                uint2 *__restrict__ list, unsigned cap, unsigned *__restrict__ count)
{
    extern __shared__ uint4 spz_lds[];
    __shared__ int off[SPZ_FIELDS];                              // the layout's offsets (dynamic indices: LDS, not SGPRs)
    if ((int)threadIdx.x < SPZ_FIELDS) off[threadIdx.x] = L.off[threadIdx.x];
    const int tr = blockDim.x, rb = L.row_bytes;
    const size_t in_bytes = spz_in_bytes(tr, rb);
    unsigned char *img = reinterpret_cast<unsigned char *>(spz_lds) + in_bytes;
    const unsigned *in32 = reinterpret_cast<const unsigned *>(spz_lds);
    // section s of the tile image: tr * width[s] bytes from img + tr * start[s]
    const int width[6] = {9, 1, 3, 3, 4, 3 * sh_dim};
    const int start[6] = {0, 9, 10, 13, 16, 20};
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();                                         // the previous tile's image has been written out
        const int base = spz_stage_tile(rows, rb, t0, cnt, spz_lds);
        __syncthreads();
        const int r = threadIdx.x;
        if (r < cnt) {
            const int q = base + r * rb;
            auto fld = [&](int f) { return lds_f32(in32, q + off[f]); };
            const int64_t row = t0 + r;
            // positions (:111-116): round(v * 4096) -> int32 -> the low 24 bits, little-endian
            unsigned char *p = img + 9 * r;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int c = spz_f32_to_i32(rintf(__fmul_rn(fld(a), 4096.0f)));
                p[3 * a] = (unsigned char)c;
                p[3 * a + 1] = (unsigned char)(c >> 8);
                p[3 * a + 2] = (unsigned char)(c >> 16);
            }
            // alpha (:118-124): (1 / (1 + exp(-clip(o, -20, 20))) * 255).astype(u8), default 255
            unsigned alpha = 255u;
            if (off[SPZ_F_OPACITY] >= 0) {
                const float o = fld(SPZ_F_OPACITY);
                const float oc = o == o ? fminf(fmaxf(o, -20.0f), 20.0f) : o;
                bool ok;
                alpha = sog_alpha_texel(oc, &ok);
                if (!ok) {
                    alpha = 0u;
                    list_append(list, cap, count, (unsigned)row, 0u);
                }
            }
            img[tr * 9 + r] = (unsigned char)alpha;
            // colours (:126-134): clip((dc * 0.15 + 0.5) * 255, 0, 255).astype(u8), default 128
            unsigned char *pc = img + tr * 10 + 3 * r;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                unsigned v = 128u;
                if (off[SPZ_F_DC] >= 0) v = spz_u8(__fmul_rn(__fadd_rn(__fmul_rn(fld(SPZ_F_DC + a), (float)0.15), 0.5f), 255.0f));
                pc[a] = (unsigned char)v;
            }
            // scales (:136-141): clip((s + 10) * 16, 0, 255).astype(u8)
            unsigned char *ps = img + tr * 13 + 3 * r;
#pragma unroll
            for (int a = 0; a < 3; ++a) ps[a] = (unsigned char)spz_u8(__fmul_rn(__fadd_rn(fld(SPZ_F_SCALE + a), 10.0f), 16.0f));
            // rotations (:143-146, :298-343)
            bool host;
            const unsigned word = spz_rot_word(fld(SPZ_F_ROT), fld(SPZ_F_ROT + 1), fld(SPZ_F_ROT + 2), fld(SPZ_F_ROT + 3), &host);
            *reinterpret_cast<unsigned *>(img + tr * 16 + 4 * r) = word;
            if (host) list_append(list, cap, count, (unsigned)row, 1u);
            // SH (:148-170): coefficient i of channel c is f_rest_{i + 15 c}; the first 9 interleaved values 5 bits, the rest 4
            unsigned char *ph = img + tr * 20 + 3 * sh_dim * r;
            for (int i = 0; i < sh_dim; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int k = 3 * i + c;
                    ph[k] = (unsigned char)spz_sh_byte(fld(SPZ_F_REST + i + 15 * c), k < 9 ? 3 : 4);
                }
            }
        }
        __syncthreads();
        // every section slice -> its span of the body: bytes up to a 16-byte boundary, 16-byte stores, the tail bytes
#pragma unroll 1
        for (int s = 0; s < 6; ++s) {
            const int w = width[s];
            if (w == 0) continue;
            const int64_t g0 = (int64_t)start[s] * n + t0 * w;
            store_bytes(out, g0, g0 + (int64_t)cnt * w, img + tr * start[s]);
        }
    }
}

// the shared checks, then SPZ's own: x .. scale_2 required, f_dc_0..2 together, the SH degree's f_rest fields present
static int spz_layout(const gsx_spz_layout *l, int sh_dim, SpzLayoutDev *out, const char *who)
{
    GSX_CHECK(layout_to_dev(l, fields_below(SPZ_F_DC), out, who));
    if ((out->off[SPZ_F_DC] >= 0) && (out->off[SPZ_F_DC + 1] < 0 || out->off[SPZ_F_DC + 2] < 0)) GSX_FAIL("%s: f_dc_0 without f_dc_1 / f_dc_2", who);
    for (int i = 0; i < sh_dim; ++i)
        for (int c = 0; c < 3; ++c)
            if (out->off[SPZ_F_REST + i + 15 * c] < 0) GSX_FAIL("%s: f_rest_%d is absent", who, i + 15 * c);
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_spz_rest_nonzero_dev(gsx_ctx *c, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, uint64_t fields, uint64_t *mask_out)
{
    if (!c || !mask_out || (n > 0 && !rows_dev)) GSX_FAIL("gsx_spz_rest_nonzero_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_spz_rest_nonzero_dev: 0 <= n < 2^32");
    if (fields >> 45) GSX_FAIL("gsx_spz_rest_nonzero_dev: fields beyond f_rest_44");
    if (reinterpret_cast<uintptr_t>(rows_dev) & 15) GSX_FAIL("gsx_spz_rest_nonzero_dev: rows must be 16-byte aligned");
    SpzLayoutDev L;
    GSX_CHECK(spz_layout(layout, 0, &L, "gsx_spz_rest_nonzero_dev"));
    RestOffsets O;
    for (int i = 0; i < 45; ++i) {
        if (((fields >> i) & 1) && L.off[SPZ_F_REST + i] < 0) GSX_FAIL("gsx_spz_rest_nonzero_dev: f_rest_%d is absent", i);
        O.off[i] = L.off[SPZ_F_REST + i];
    }
    GSX_HIP(hipSetDevice(c->device));
    *mask_out = 0;
    if (n == 0 || fields == 0) return 0;
    return rest_scan(c, rows_dev, L.row_bytes, n, O, fields, mask_out);
}

int gsx_spz_pack_dev(gsx_ctx *c, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int sh_degree, uint8_t *body_dev,
                     uint32_t *list_dev, int64_t cap, uint32_t *count_dev)
{
    if (!c || !count_dev || (n > 0 && (!rows_dev || !body_dev)) || (cap > 0 && !list_dev)) GSX_FAIL("gsx_spz_pack_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_spz_pack_dev: 0 <= n < 2^32");
    if (sh_degree < 0 || sh_degree > 3) GSX_FAIL("gsx_spz_pack_dev: SH degree %d (0 ... 3)", sh_degree);
    if (cap < 0 || cap > 0xffffffffLL) GSX_FAIL("gsx_spz_pack_dev: bad list capacity");
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(body_dev) & 15))
        GSX_FAIL("gsx_spz_pack_dev: rows and body must be 16-byte aligned");
    const int sh_dim = spz_sh_dim(sh_degree);
    SpzLayoutDev L;
    GSX_CHECK(spz_layout(layout, sh_dim, &L, "gsx_spz_pack_dev"));
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipMemsetAsync(count_dev, 0, 4, c->stream));
    if (n == 0) return 0;
    const int tr = spz_tile_rows(L.row_bytes);
    const size_t lds = spz_in_bytes(tr, L.row_bytes) + (size_t)tr * spz_row_out_bytes(sh_dim) + 32;
    hipLaunchKernelGGL(spz_pack_kernel, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), lds, c->stream, static_cast<const uint4 *>(rows_dev), L, n, sh_dim,
                       body_dev, reinterpret_cast<uint2 *>(list_dev), (unsigned)cap, count_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
