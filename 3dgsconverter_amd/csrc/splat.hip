// splat.hip -- numeric core of the .splat writer: one 32-byte record per row, in the order of np.argsort(-metric) with ties
// kept in input order, from the raw rows of a splat table.
//
// Replaces, in gsconverter/formats/splat.py (SplatFormat.write):
//   visibility metric      :92-94    exp((s0 + s1) + s2) * (1 / (1 + exp(-opacity)))               -> splat_pack_kernel (the key)
//   sort                   :98       np.argsort(-metric)                                             -> gsx_splat_order_dev (stable)
//   reorder                :101      data[sorted_indices]                                            -> splat_permute_kernel
//   record fields          :104-161  position bits, np.exp(scale), colour / alpha u8, rotation u8    -> splat_pack_kernel
//
// The records are packed in INPUT order (one coalesced pass over the rows, tiles staged in LDS by row_tile.h), next to a u32
// key per row; a stable radix sort of (key, row index) gives the order, and the permute pass moves 32-byte records, not the
// 248-byte rows.  The key of v = -metric is the usual order-preserving map of float32 to u32, after -0 -> +0 (numpy compares
// them equal) and every NaN -> 0xffffffff (numpy sorts NaN after every number; NaNs compare equal among themselves).  Equal
// keys keep input order: np.argsort(-metric, kind="stable").
//
// Every float32 operation is numpy's, in numpy's order (the library is built with -ffp-contract=off); exp is numpy's own SIMD
// exp (np_exp.h).  A NaN reaching a float -> u8 cast gives 0, numpy's result on x86 (spz_u8; the golden edge rows pin it).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "gsx_common.h"
#include "np_exp.h"
#include "row_tile.h"
#include "sog_math.h"
#include "splat_metric.h"

namespace gsx {

constexpr int SPLAT_REC = 32;   // bytes per record: 3 f32 position | 3 f32 scale | 4 u8 colour | 4 u8 rotation

struct SplatRgb {
    int off[3];   // byte offsets of the u1 fields red, green, blue; off[0] < 0: colour from f_dc_0..2
};

// :92-94 -> the key of -metric
template <class Fld>
__device__ __forceinline__ unsigned splat_metric_key(Fld fld)
{
    return splat_metric_key_of(fld(SPZ_F_SCALE), fld(SPZ_F_SCALE + 1), fld(SPZ_F_SCALE + 2), fld(SPZ_F_OPACITY));
}

// :104-161 -> the record's eight words.  byte(k): the k-th colour byte (red, green, blue) in the fallback of :140-143
template <class Fld, class Byte>
__device__ __forceinline__ void splat_record(Fld fld, Byte byte, bool rgb, unsigned w[8])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = __float_as_uint(fld(a));                            // :150 positions
#pragma unroll
    for (int a = 0; a < 3; ++a) w[3 + a] = __float_as_uint(np_expf(fld(SPZ_F_SCALE + a)));   // :109 np.exp of the scales
    unsigned col = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        unsigned c;
        if (rgb) {
            c = byte(a);                                                                    // :140-143
        } else {                                                                            // :134-138
            c = spz_u8(__fmul_rn(__fadd_rn(0.5f, __fmul_rn((float)0.28209479177387814, fld(SPZ_F_DC + a))), 255.0f));
        }
        col |= c << (8 * a);
    }
    {                                                                                       // :145 alpha
        const float e = np_expf(-fld(SPZ_F_OPACITY));
        col |= spz_u8(__fmul_rn(__fdiv_rn(1.0f, __fadd_rn(1.0f, e)), 255.0f)) << 24;
    }
    w[6] = col;
    // :115-128 rotations: norms = sqrt(((r0^2 + r1^2) + r2^2) + r3^2), r /= norms, clip(r * 128 + 128, 0, 255) -> u8
    float r[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) r[a] = fld(SPZ_F_ROT + a);
    float ss = __fmul_rn(r[0], r[0]);
#pragma unroll
    for (int a = 1; a < 4; ++a) ss = __fadd_rn(ss, __fmul_rn(r[a], r[a]));
    const float norm = __builtin_sqrtf(ss);   // correctly rounded (HIP's __fsqrt_rn is the native v_sqrt_f32 here, 1 ulp off at times)
    unsigned rot = 0u;
#pragma unroll
    for (int a = 0; a < 4; ++a) rot |= spz_u8(__fadd_rn(__fmul_rn(__fdiv_rn(r[a], norm), 128.0f), 128.0f)) << (8 * a);
    w[7] = rot;
}

__device__ __forceinline__ void splat_store(unsigned char *__restrict__ recs, int64_t i, const unsigned w[8])
{
    uint4 *o = reinterpret_cast<uint4 *>(recs + i * SPLAT_REC);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// rows in input order -> keys[i] and the record of row i at recs + 32 i; a workgroup stages a tile of rows in LDS
__global__ void splat_pack_kernel(const uint4 *__restrict__ rows, SpzLayoutDev L, SplatRgb C, int64_t n, unsigned *__restrict__ keys,
                                  unsigned char *__restrict__ recs)
{
    extern __shared__ uint4 sp_lds[];
    __shared__ int off[SPZ_FIELDS];
    if ((int)threadIdx.x < SPZ_FIELDS) off[threadIdx.x] = L.off[threadIdx.x];
    const int tr = blockDim.x, rb = L.row_bytes;
    const unsigned *in32 = reinterpret_cast<const unsigned *>(sp_lds);
    const bool rgb = C.off[0] >= 0;
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();                                         // the previous tile has been read
        const int base = spz_stage_tile(rows, rb, t0, cnt, sp_lds);
        __syncthreads();
        const int r = threadIdx.x;
        if (r < cnt) {
            const int q = base + r * rb;
            auto fld = [&](int f) { return lds_f32(in32, q + off[f]); };
            auto byte = [&](int k) { return lds_u8(in32, q + C.off[k]); };
            const int64_t row = t0 + r;
            keys[row] = splat_metric_key(fld);
            unsigned w[8];
            splat_record(fld, byte, rgb, w);
            splat_store(recs, row, w);
        }
    }
}

// the same arithmetic on rows read in place: keys only (order == nullptr, recs == nullptr), or the record of row order[i] at
// recs + 32 i (the sort-first variant: records gathered from the raw rows in sorted order)
__global__ __launch_bounds__(256) void splat_direct_kernel(const unsigned char *__restrict__ rows, SpzLayoutDev L, SplatRgb C, int64_t n,
                                                           const unsigned *__restrict__ order, unsigned *__restrict__ keys,
                                                           unsigned char *__restrict__ recs)
{
    const bool rgb = C.off[0] >= 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = order ? (int64_t)order[i] : i;
        const int64_t rowb = row * L.row_bytes;
        auto fld = [&](int f) { return ld_f32(rows, rowb + L.off[f]); };
        auto byte = [&](int k) { return (unsigned)rows[rowb + C.off[k]]; };
        if (keys) keys[i] = splat_metric_key(fld);
        if (recs) {
            unsigned w[8];
            splat_record(fld, byte, rgb, w);
            splat_store(recs, i, w);
        }
    }
}

// metric -> key of -metric (the key-order proof of the GPU tests, and the host-exp path: numpy's metric, the device's sort)
__global__ __launch_bounds__(256) void splat_keys_kernel(const float *__restrict__ metric, int64_t n, unsigned *__restrict__ keys)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        keys[i] = sort_key(-metric[i]);
}

// out[i] = recs[order[i]]: two lanes per record, one 16-byte load and one 16-byte store each; the stores are contiguous
__global__ __launch_bounds__(256) void splat_permute_kernel(const uint4 *__restrict__ recs, const unsigned *__restrict__ order, int64_t n,
                                                            uint4 *__restrict__ out)
{
    const int64_t m = 2 * n;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x)
        out[j] = recs[2 * (int64_t)order[j >> 1] + (j & 1)];
}

// the shared checks (x .. scale_2 and opacity required, f_dc_0..2 too without colour bytes), then the colour bytes' own
static int splat_layout(const gsx_spz_layout *l, const int rgb[3], SpzLayoutDev *out, SplatRgb *c, const char *who)
{
    const bool from_dc = rgb[0] < 0;
    GSX_CHECK(layout_to_dev(l, fields_below(from_dc ? SPZ_F_REST : SPZ_F_DC) | 1ull << SPZ_F_OPACITY, out, who));
    if (!from_dc && (rgb[1] < 0 || rgb[2] < 0)) GSX_FAIL("%s: red, green and blue offsets go together", who);
    for (int k = 0; k < 3; ++k) {
        if (!from_dc && rgb[k] >= l->row_bytes) GSX_FAIL("%s: colour byte %d at offset %d of a %lld-byte row", who, k, rgb[k], (long long)l->row_bytes);
        c->off[k] = from_dc ? -1 : rgb[k];
    }
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_splat_pack_dev(gsx_ctx *c, const void *rows_dev, const gsx_spz_layout *layout, int red_off, int green_off, int blue_off, int64_t n,
                       const uint32_t *order_dev, uint32_t *keys_dev, uint8_t *recs_dev)
{
    if (!c || (n > 0 && (!rows_dev || (!keys_dev && !recs_dev)))) GSX_FAIL("gsx_splat_pack_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_splat_pack_dev: 0 <= n < 2^32");
    if (order_dev && (keys_dev || !recs_dev)) GSX_FAIL("gsx_splat_pack_dev: an order gathers records only");
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(recs_dev) & 15) || (reinterpret_cast<uintptr_t>(keys_dev) & 3))
        GSX_FAIL("gsx_splat_pack_dev: rows and records must be 16-byte aligned, keys 4-byte aligned");
    const int rgb[3] = {red_off, green_off, blue_off};
    SpzLayoutDev L;
    SplatRgb C;
    GSX_CHECK(splat_layout(layout, rgb, &L, &C, "gsx_splat_pack_dev"));
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    if (order_dev || !recs_dev || !keys_dev) {
        hipLaunchKernelGGL(splat_direct_kernel, dim3(tile_blocks(c, n, 256, 16)), dim3(256), 0, c->stream, static_cast<const unsigned char *>(rows_dev),
                           L, C, n, order_dev, keys_dev, recs_dev);
    } else {
        const int tr = spz_tile_rows(L.row_bytes);
        hipLaunchKernelGGL(splat_pack_kernel, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), spz_in_bytes(tr, L.row_bytes), c->stream,
                           static_cast<const uint4 *>(rows_dev), L, C, n, keys_dev, recs_dev);
    }
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_splat_keys_dev(gsx_ctx *c, const float *metric_dev, int64_t n, uint32_t *keys_dev)
{
    if (!c || (n > 0 && (!metric_dev || !keys_dev))) GSX_FAIL("gsx_splat_keys_dev: null argument");
    if (n < 0) GSX_FAIL("gsx_splat_keys_dev: n < 0");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(splat_keys_kernel, dim3(tile_blocks(c, n, 256, 16)), dim3(256), 0, c->stream, metric_dev, n, keys_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_splat_order_dev(gsx_ctx *c, const uint32_t *keys_dev, int64_t n, uint32_t *order_dev)
{
    if (!c || (n > 0 && (!keys_dev || !order_dev))) GSX_FAIL("gsx_splat_order_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_splat_order_dev: 0 <= n < 2^32");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    rocprim::counting_iterator<unsigned> iota(0u);
    size_t temp_bytes = 0;
    unsigned *nul = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_dev, nul, iota, nul, (size_t)n, 0, 32, c->stream) != hipSuccess)
        GSX_FAIL("gsx_splat_order_dev: rocprim size query failed");
    const size_t col = sizeof(unsigned) * (size_t)n;
    GSX_CHECK(c->splat_sort.reserve(col + temp_bytes + 512));
    unsigned *keys_out = c->splat_sort.as<unsigned>();
    void *temp = reinterpret_cast<void *>((reinterpret_cast<uintptr_t>(keys_out + n) + 255) & ~(uintptr_t)255);
    GSX_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, keys_dev, keys_out, iota, order_dev, (size_t)n, 0, 32, c->stream));   // stable
    return 0;
}

int gsx_splat_permute_dev(gsx_ctx *c, const uint8_t *recs_dev, const uint32_t *order_dev, int64_t n, uint8_t *out_dev)
{
    if (!c || (n > 0 && (!recs_dev || !order_dev || !out_dev))) GSX_FAIL("gsx_splat_permute_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_splat_permute_dev: 0 <= n < 2^32");
    if ((reinterpret_cast<uintptr_t>(recs_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        GSX_FAIL("gsx_splat_permute_dev: records must be 16-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(splat_permute_kernel, dim3(tile_blocks(c, 2 * n, 256, 16)), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(recs_dev),
                       order_dev, n, reinterpret_cast<uint4 *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
