// ksplat.hip -- numeric core of the .ksplat writer: the bucket centres and every interleaved row of the payload, from the raw
// rows of a splat table.
//
// Replaces, in gsconverter/formats/ksplat.py (KSplatFormat.write):
//   bucket centres         :426-450  np.minimum/maximum.reduceat per bucket, (min + max) / 2.0    -> ksplat_centre_kernel (+ _finish)
//   quantised positions    :452-457  clip(round((x - c) * sf_inv) + 32767, 0, 65535) -> u16       -> ksplat_pack_kernel
//   scales, rotations      :463-475  np.exp of the scales, float32 or float16                    -> ksplat_pack_kernel
//   colour and alpha       :477-483                                                                -> ksplat_pack_kernel
//   SH, interleaving       :485-536  f_rest_0.. as float32 / float16 / the u8 quantiser (level 2) / a bare u8 cast
//                                     (levels >= 3: :527-533 skip the quantiser), per row            -> ksplat_pack_kernel
// (the SH degree of :340-368 is gsx_spz_rest_nonzero_dev's scan, csrc/spz.hip)
//
// The payload behind the two headers is  [u32 N % bucket_size] | [bucket_count x 3 f32 centres, levels >= 1] | N rows of
// bytes_per_splat.  Centres: one pass over x, y, z in tiles of KS_CT rows; a bucket that lies wholly inside a tile is reduced
// there (LDS), a bucket that straddles tiles is combined through order-preserving integer atomics in a slot owned by its first
// tile, and ksplat_finish_kernel completes those.  Rows: a workgroup stages a tile of raw rows in LDS (row_tile.h), packs each
// row into an LDS image of the tile's output rows, and writes that image as ONE contiguous span with 16-byte stores (byte
// stores at the two unaligned ends: rows of 33, 42, 72, 80 or 140 bytes never start a tile aligned).
//
// Every float32 operation is numpy's, in numpy's order (the library is built with -ffp-contract=off); exp is numpy's own SIMD
// exp (np_exp.h), the f16 casts are __float2half_rn (numpy's astype(float16) for every non-NaN input).  Results that depend on
// how numpy's x86 casts treat a NaN are left to the host, listed as (index, kind) in `list`:
//   kind 0  row i: a NaN reaches a float -> u8 / u16 cast (position, colour, alpha, SH at levels >= 2) or a float -> f16 cast
//   kind 2  bucket i: its centre is NaN, or an axis holds only zeros of both signs (numpy's reduction order picks the sign)
#include <hip/hip_fp16.h>

#include "gsx_common.h"
#include "np_exp.h"
#include "row_tile.h"
#include "sog_math.h"

namespace gsx {

constexpr int KS_CT = 256;                 // rows per tile (= threads) of the centre kernel
constexpr unsigned KS_KEY_NEG0 = 0x7fffffffu, KS_KEY_POS0 = 0x80000000u;   // float_key(-0.0f), float_key(+0.0f)
constexpr unsigned KS_KIND_ROW = 0u, KS_KIND_BUCKET = 2u;

// a bucket's centre from its keys: (min + max) / 2.0 per axis in float32 (:440-444), straight into the payload
__device__ void ks_finish_bucket(int64_t b, const unsigned mn[3], const unsigned mx[3], unsigned flag, float *centres, uint2 *list,
                                 unsigned cap, unsigned *count)
{
    bool host = flag != 0u;                                       // a NaN among the bucket's values
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        host |= mn[a] == KS_KEY_NEG0 && mx[a] == KS_KEY_POS0;     // only zeros, both signs
        const float c = __fdiv_rn(__fadd_rn(sort_unkey(mn[a]), sort_unkey(mx[a])), 2.0f);
        host |= c != c;                                           // -inf + inf: numpy's NaN bits are x86's
        centres[3 * b + a] = c;
    }
    if (host) list_append(list, cap, count, (unsigned)b, KS_KIND_BUCKET);
}

__device__ __forceinline__ unsigned ks_wave_min(unsigned v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, s, 64));
    return v;
}

__device__ __forceinline__ unsigned ks_wave_max(unsigned v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, s, 64));
    return v;
}

// gmin: 3 keys per tile (memset 0xff), gmax: 3 keys + 1 flag word per tile (memset 0) -- the slots of straddling buckets
__global__ __launch_bounds__(KS_CT) void ksplat_centre_kernel(const unsigned char *__restrict__ rows, int rb, int ox, int oy, int oz,
                                                              int64_t n, int64_t B, float *__restrict__ centres,
                                                              unsigned *__restrict__ gmin, unsigned *__restrict__ gmax, uint2 *__restrict__ list,
                                                              unsigned cap, unsigned *__restrict__ count)
{
    __shared__ unsigned smin[3][KS_CT], smax[3][KS_CT], sflag[KS_CT];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t ntiles = (n + KS_CT - 1) / KS_CT;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * KS_CT;
        const int cnt = (int)min((int64_t)KS_CT, n - t0);
        const int64_t b_lo = t0 / B;
        const int nloc = (int)((t0 + cnt - 1) / B - b_lo) + 1;   // <= KS_CT buckets touch the tile
        __syncthreads();                                         // the previous tile's slots have been read
        for (int j = t; j < nloc; j += KS_CT) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                smin[a][j] = 0xffffffffu;
                smax[a][j] = 0u;
            }
            sflag[j] = 0u;
        }
        __syncthreads();
        unsigned kmin[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, kmax[3] = {0u, 0u, 0u}, nan = 0u;
        int64_t b = -1;
        if (t < cnt) {
            const int64_t row = t0 + t, rowb = row * rb;
            const float v[3] = {ld_f32(rows, rowb + ox), ld_f32(rows, rowb + oy), ld_f32(rows, rowb + oz)};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (v[a] != v[a]) {
                    nan = 1u;
                } else {
                    kmin[a] = kmax[a] = float_key(v[a]);
                }
            }
            b = row / B;
        }
        // a wave whose rows all fall in one bucket (bucket_size >= 64, the usual case) combines in registers first
        const int64_t w0 = t0 + (t - lane);
        const int64_t wl = min(w0 + 63, t0 + cnt - 1);
        const bool uniform = w0 <= wl && w0 / B == wl / B;        // wave-uniform
        if (uniform) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                kmin[a] = ks_wave_min(kmin[a]);
                kmax[a] = ks_wave_max(kmax[a]);
            }
            nan = ks_wave_max(nan);
        }
        if (b >= 0 && (!uniform || lane == 0)) {
            const int j = (int)(b - b_lo);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(&smin[a][j], kmin[a]);
                atomicMax(&smax[a][j], kmax[a]);
            }
            if (nan) atomicOr(&sflag[j], 1u);
        }
        __syncthreads();
        for (int j = t; j < nloc; j += KS_CT) {
            const int64_t bb = b_lo + j, bs = bb * B, be = min(bs + B, n);
            const unsigned mn[3] = {smin[0][j], smin[1][j], smin[2][j]}, mx[3] = {smax[0][j], smax[1][j], smax[2][j]};
            if (bs >= t0 && be <= t0 + cnt) {
                ks_finish_bucket(bb, mn, mx, sflag[j], centres, list, cap, count);
            } else {                                             // straddles tiles: the slot of its first tile
                const int64_t s = bs / KS_CT;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    atomicMin(&gmin[3 * s + a], mn[a]);
                    atomicMax(&gmax[4 * s + a], mx[a]);
                }
                if (sflag[j]) atomicOr(&gmax[4 * s + 3], 1u);
            }
        }
    }
}

// the straddling buckets: the one whose first tile is tile k, if any, is the bucket of tile k's last row
__global__ void ksplat_finish_kernel(int64_t n, int64_t B, float *__restrict__ centres, const unsigned *__restrict__ gmin,
                                     const unsigned *__restrict__ gmax, uint2 *__restrict__ list, unsigned cap, unsigned *__restrict__ count)
{
    const int64_t ntiles = (n + KS_CT - 1) / KS_CT;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < ntiles; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t0 = k * KS_CT, t1 = min(t0 + KS_CT, n);
        const int64_t b = (t1 - 1) / B, bs = b * B, be = min(bs + B, n);
        if (bs < t0 || be <= t1) continue;                       // starts in an earlier tile, or lies wholly in this one
        const unsigned mn[3] = {gmin[3 * k], gmin[3 * k + 1], gmin[3 * k + 2]}, mx[3] = {gmax[4 * k], gmax[4 * k + 1], gmax[4 * k + 2]};
        ks_finish_bucket(b, mn, mx, gmax[4 * k + 3], centres, list, cap, count);
    }
}

struct KsPackArgs {
    int level;          // 0, 1, 2, or 3 (every level >= 3 writes the same body)
    int sh_count;       // 0, 9, 24: f_rest_0 .. f_rest_{sh_count-1}, in index order (:488)
    int bps;            // bytes per output row
    int64_t bucket;     // bucket_size (levels >= 1)
    float sf;           // float32(32767 / (block_size / 2.0)) (:455)
    int64_t row_base;   // byte offset of row 0 in the payload
};

__device__ __forceinline__ void ks_put(unsigned char *p, unsigned v, int bytes)
{
    for (int i = 0; i < bytes; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

// numpy's float32 -> uint8 cast on x86 without a clip: the low byte of the truncated int32 (cvttss2si), 0 where that is
// INT_MIN (|v| >= 2^31, +-inf; NaN is listed)
__device__ __forceinline__ unsigned ks_f32_to_u8_wrap(float v)
{
    return (v > -2147483648.0f && v < 2147483648.0f) ? ((unsigned)(int)v & 0xffu) : 0u;
}

__device__ __forceinline__ unsigned ks_half(float v) { return (unsigned)__half_as_ushort(__float2half_rn(v)); }

// rows -> the tile's interleaved output rows, written as one span of the payload
__global__ void ksplat_pack_kernel(const uint4 *__restrict__ rows, SpzLayoutDev L, int64_t n, KsPackArgs P, const float *__restrict__ centres,
                                   unsigned char *__restrict__ payload, uint2 *__restrict__ list, unsigned cap, unsigned *__restrict__ count)
{
    extern __shared__ uint4 ks_lds[];
    __shared__ int off[SPZ_FIELDS];
    if ((int)threadIdx.x < SPZ_FIELDS) off[threadIdx.x] = L.off[threadIdx.x];
    const int tr = blockDim.x, rb = L.row_bytes, bps = P.bps;
    unsigned char *img = reinterpret_cast<unsigned char *>(ks_lds) + spz_in_bytes(tr, rb);
    const unsigned *in32 = reinterpret_cast<const unsigned *>(ks_lds);
    const int pw = P.level == 0 ? 4 : 2;                         // bytes per position / scale / rotation item
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();                                         // the previous tile's image has been written out
        const int base = spz_stage_tile(rows, rb, t0, cnt, ks_lds);
        __syncthreads();
        const int r = threadIdx.x;
        if (r < cnt) {
            const int q = base + r * rb;
            auto fld = [&](int f) { return lds_f32(in32, q + off[f]); };
            const int64_t row = t0 + r;
            unsigned char *o = img + r * bps;
            bool host = false;
            // positions (:452-458): float32 as they are, or quantised against the bucket's centre
            if (P.level == 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) ks_put(o + 4 * a, __float_as_uint(fld(a)), 4);
            } else {
                const float *c = centres + 3 * (row / P.bucket);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float v = rintf(__fmul_rn(__fsub_rn(fld(a), c[a]), P.sf));
                    v = __fadd_rn(v, 32767.0f);
                    host |= v != v;
                    ks_put(o + 2 * a, v == v ? (unsigned)fminf(fmaxf(v, 0.0f), 65535.0f) : 0u, 2);
                }
            }
            o += 3 * pw;
            // scales (:463-468): np.exp, as float32 bits or cast to float16
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float e = np_expf(fld(SPZ_F_SCALE + a));
                if (P.level == 0) {
                    ks_put(o + 4 * a, __float_as_uint(e), 4);
                } else {
                    host |= e != e;
                    ks_put(o + 2 * a, ks_half(e), 2);
                }
            }
            o += 3 * pw;
            // rotations (:470-475): rot_0..3 as they are, or cast to float16
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float v = fld(SPZ_F_ROT + a);
                if (P.level == 0) {
                    ks_put(o + 4 * a, __float_as_uint(v), 4);
                } else {
                    host |= v != v;
                    ks_put(o + 2 * a, ks_half(v), 2);
                }
            }
            o += 4 * pw;
            // colour (:477-483): clip((0.5 + SH_C0 * f_dc) * 255, 0, 255) -> u8; alpha clip((1 / (1 + exp(-opacity))) * 255, 0, 255) -> u8
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v = __fmul_rn(__fadd_rn(0.5f, __fmul_rn((float)0.28209479177387814, fld(SPZ_F_DC + a))), 255.0f);
                host |= v != v;
                o[a] = (unsigned char)spz_u8(v);
            }
            {
                const float e = np_expf(-fld(SPZ_F_OPACITY));
                const float v = __fmul_rn(__fdiv_rn(1.0f, __fadd_rn(1.0f, e)), 255.0f);
                host |= v != v;
                o[3] = (unsigned char)spz_u8(v);
            }
            o += 4;
            // SH (:485-497, :527-531): f_rest_0 .. f_rest_{sh_count-1} as float32, float16, or clip((v + 2) / 4 * 255, 0, 255) -> u8
            for (int j = 0; j < P.sh_count; ++j) {
                const float v = fld(SPZ_F_REST + j);
                if (P.level == 0) {
                    ks_put(o + 4 * j, __float_as_uint(v), 4);
                } else if (P.level == 1) {
                    host |= v != v;
                    ks_put(o + 2 * j, ks_half(v), 2);
                } else if (P.level == 2) {
                    const float s = __fmul_rn(__fdiv_rn(__fsub_rn(v, -2.0f), 4.0f), 255.0f);
                    host |= s != s;
                    o[j] = (unsigned char)spz_u8(s);
                } else {                                           // levels >= 3: astype(np.uint8) of the value itself (:533)
                    host |= v != v;
                    o[j] = (unsigned char)ks_f32_to_u8_wrap(v);
                }
            }
            if (host) list_append(list, cap, count, (unsigned)row, KS_KIND_ROW);
        }
        __syncthreads();
        // the tile's rows -> their span of the payload: bytes up to a 16-byte boundary, 16-byte stores, the tail bytes
        const int64_t g0 = P.row_base + t0 * bps;
        store_bytes(payload, g0, g0 + (int64_t)cnt * bps, img);
    }
}

// np.exp and astype(np.float16) of every input, element by element (the devtools' proofs and the GPU tests)
__global__ void ksplat_math_kernel(const float *__restrict__ x, int64_t n, unsigned *__restrict__ e, unsigned short *__restrict__ h)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        e[i] = __float_as_uint(np_expf(v));
        h[i] = __half_as_ushort(__float2half_rn(v));
    }
}

// x .. opacity and f_rest_0 .. f_rest_{sh_count-1} are required
static uint64_t ks_required(int sh_count) { return fields_below(SPZ_F_REST + sh_count); }

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_ksplat_centres_dev(gsx_ctx *c, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int64_t bucket_size,
                           float *centres_dev, uint32_t *list_dev, int64_t cap, uint32_t *count_dev)
{
    if (!c || !count_dev || (n > 0 && (!rows_dev || !centres_dev)) || (cap > 0 && !list_dev)) GSX_FAIL("gsx_ksplat_centres_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_ksplat_centres_dev: 0 <= n < 2^32");
    if (bucket_size < 1 || bucket_size >= (1LL << 32)) GSX_FAIL("gsx_ksplat_centres_dev: bucket_size %lld (1 ... 2^32 - 1)", (long long)bucket_size);
    if (cap < 0 || cap > 0xffffffffLL) GSX_FAIL("gsx_ksplat_centres_dev: bad list capacity");
    if (reinterpret_cast<uintptr_t>(centres_dev) & 3) GSX_FAIL("gsx_ksplat_centres_dev: centres must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(rows_dev) & 15) GSX_FAIL("gsx_ksplat_centres_dev: rows must be 16-byte aligned");
    SpzLayoutDev L;
    GSX_CHECK(layout_to_dev(layout, ks_required(0), &L, "gsx_ksplat_centres_dev"));
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    const int64_t ntiles = (n + KS_CT - 1) / KS_CT;
    GSX_CHECK(c->ksplat_keys.reserve((size_t)ntiles * 7 * sizeof(unsigned)));
    unsigned *gmin = c->ksplat_keys.as<unsigned>(), *gmax = gmin + 3 * ntiles;
    GSX_HIP(hipMemsetAsync(gmin, 0xff, (size_t)ntiles * 3 * sizeof(unsigned), c->stream));
    GSX_HIP(hipMemsetAsync(gmax, 0, (size_t)ntiles * 4 * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(ksplat_centre_kernel, dim3(tile_blocks(c, n, KS_CT, 8)), dim3(KS_CT), 0, c->stream, static_cast<const unsigned char *>(rows_dev),
                       L.row_bytes, L.off[0], L.off[1], L.off[2], n, bucket_size, centres_dev, gmin, gmax, reinterpret_cast<uint2 *>(list_dev),
                       (unsigned)cap, count_dev);
    GSX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ksplat_finish_kernel, dim3(tile_blocks(c, ntiles, 256, 4)), dim3(256), 0, c->stream, n, bucket_size, centres_dev, gmin, gmax,
                       reinterpret_cast<uint2 *>(list_dev), (unsigned)cap, count_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_ksplat_pack_dev(gsx_ctx *c, const void *rows_dev, const gsx_spz_layout *layout, int64_t n, int level, int sh_count,
                        int64_t bucket_size, float sf_inv, const float *centres_dev, uint8_t *payload_dev, int64_t row_base,
                        uint32_t *list_dev, int64_t cap, uint32_t *count_dev)
{
    if (!c || !count_dev || (n > 0 && (!rows_dev || !payload_dev)) || (cap > 0 && !list_dev)) GSX_FAIL("gsx_ksplat_pack_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_ksplat_pack_dev: 0 <= n < 2^32");
    if (level < 0 || level > 3) GSX_FAIL("gsx_ksplat_pack_dev: level %d (0 ... 3)", level);
    if (sh_count != 0 && sh_count != 9 && sh_count != 24) GSX_FAIL("gsx_ksplat_pack_dev: sh_count %d (0, 9 or 24)", sh_count);
    if (level >= 1 && (bucket_size < 1 || (n > 0 && !centres_dev))) GSX_FAIL("gsx_ksplat_pack_dev: levels >= 1 need bucket_size >= 1 and centres");
    if (row_base < 0) GSX_FAIL("gsx_ksplat_pack_dev: row_base < 0");
    if (cap < 0 || cap > 0xffffffffLL) GSX_FAIL("gsx_ksplat_pack_dev: bad list capacity");
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(payload_dev) & 15))
        GSX_FAIL("gsx_ksplat_pack_dev: rows and payload must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(centres_dev) & 3) GSX_FAIL("gsx_ksplat_pack_dev: centres must be 4-byte aligned");
    SpzLayoutDev L;
    GSX_CHECK(layout_to_dev(layout, ks_required(sh_count), &L, "gsx_ksplat_pack_dev"));
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    KsPackArgs P;
    P.level = level;
    P.sh_count = sh_count;
    P.bps = level == 0 ? 44 + 4 * sh_count : 24 + (level == 1 ? 2 : 1) * sh_count;
    P.bucket = level >= 1 ? bucket_size : 1;
    P.sf = sf_inv;
    P.row_base = row_base;
    const int tr = spz_tile_rows(L.row_bytes);
    const size_t lds = spz_in_bytes(tr, L.row_bytes) + (size_t)tr * P.bps + 32;
    hipLaunchKernelGGL(ksplat_pack_kernel, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), lds, c->stream, static_cast<const uint4 *>(rows_dev), L, n, P,
                       centres_dev, payload_dev, reinterpret_cast<uint2 *>(list_dev), (unsigned)cap, count_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_ksplat_math_dev(gsx_ctx *c, const float *x_dev, int64_t n, uint32_t *exp_out_dev, uint16_t *half_out_dev)
{
    if (!c || (n > 0 && (!x_dev || !exp_out_dev || !half_out_dev))) GSX_FAIL("gsx_ksplat_math_dev: null argument");
    if (n < 0) GSX_FAIL("gsx_ksplat_math_dev: n < 0");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(ksplat_math_kernel, dim3(tile_blocks(c, n, 256, 16)), dim3(256), 0, c->stream, x_dev, n, exp_out_dev, reinterpret_cast<unsigned short *>(half_out_dev));
    GSX_HIP(hipGetLastError());
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_np_expf_host(const float *x, float *out, int64_t n)
{
    if (n > 0 && (!x || !out)) GSX_FAIL("gsx_np_expf_host: null argument");
    for (int64_t i = 0; i < n; ++i) out[i] = np_expf(x[i]);
    return 0;
}

}  // extern "C"
