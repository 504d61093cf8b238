// render.hip -- the preview image (--preview): a tile-based forward rasteriser of 3D Gaussian splats.  No counterpart in the
// reference; the definition is tests/render_numpy.py, and every sum, product, division and root here is that
// file's, in its order: the per-splat stage float64 rounded once per operation (the build's -ffp-contract=off: no fma is written
// here), division and root correctly rounded (__ddiv_rn, __dsqrt_rn), the per-pixel stage float32 through the _rn intrinsics,
// the float32 exp of np_exp.h in both.
//
//   gsx_rows_render_work_dev   bytes of the fixed workspace for n rows and a width x height image
//   gsx_rows_render_plan_dev   (a) project  (b) count + scan; the one readback of the step
//   gsx_rows_render_draw_dev   (c) emit  (d) stable order  (e) tile ranges  (f) blend
//   gsx_rows_render_score_dev  (c) (d) (e) as above, then (g) score: what every row contributed to the pixels
//   gsx_view_keys_dev          the ranking key of a row's summed contribution (view_key.h)
//
// (a) one lane per row: the eleven geometry fields and the colour source from the packed rows where they lie (any stride, any first
//     byte) -> a record of 16 words (centre, conic, opacity, colour, depth, the pixel rectangle, visible); an invisible row's
//     record is all zero.
// (b) one lane per row: the 16 x 16 tiles its rectangle touches, as a 64-bit count; one exclusive scan gives every row the place of
//     its first instance and the total.
// (c) one lane per row writes its (tile << 32 | depth bits, row) instances from that place on, tiles in raster order: instances
//     are in row order.
// (d) rocprim's stable radix sort of the keys, over the bits the tile count needs: a tile's instances follow one another by
//     depth, equal depths in row order -- the definition's order.
// (e) one lane per sorted instance marks where its tile's run starts and ends.
// (f) one workgroup of 256 lanes per tile, one pixel per lane (a wave owns a 16 x 4 strip).  The tile's records are staged in LDS
//     in batches of 256, four lanes per 64-byte record; every lane then reads the same record, a broadcast.  The rectangle test
//     is per pixel, so a pixel never receives a splat whose rectangle misses it, whatever the tile size.  A lane whose pixel is
//     finished or outside the image adds nothing more; a wave leaves a batch and the workgroup leaves the loop when all their
//     lanes are finished -- lanes only ever stop adding, so this is the per-pixel stop rule.
//
// (g) the blend's loop with the colour left out: per (pixel, splat) pair the weight alpha * T the colour sum uses.  256 lanes hold a
//     weight for the same record at once; a wave whose ballot of contributing lanes is empty moves on, else it reduces the
//     float bits (non-negative floats order as their bits) by max and the weights' 24-bit fixed-point truncations by sum, and
//     its first lane adds both to the record's two LDS words.  After the batch, lane t sends record t's words on: at most
//     one global atomicMax (u32) and one atomicAdd (u64) per (tile, record), none when the record added nothing.  Integer
//     atomics only: the result does not depend on arrival order.
//
// The one shortcut: a splat with power < -5.6 is skipped without evaluating E.  E is numpy's float32 exp, within 2 ulp of the
// nearest float32 of exp (np_exp.h: verified over all 2^32 inputs), so E(power) < exp(-5.6) (1 + 3e-7) < 0.0036980 for every such
// power; the opacity is 1 / (1 + E(.)) <= 1 and the product is rounded once, so alpha < 0.0036981 < 1/255 = 0.0039215...: the
// definition skips that splat too.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "np_exp.h"
#include "row_tile.h"
#include "view_key.h"

namespace gsx {

constexpr int RND_TILE = GSX_RENDER_TILE;        // pixels per tile side: 256 lanes, one pixel each
constexpr int RND_BATCH = 256;                   // records staged per round
constexpr int RND_QUADS = GSX_RENDER_RECORD_WORDS / 4;
constexpr float RND_POWER_CUT = -5.6f;           // below: alpha < 1/255 whatever E's last bits are (the header comment)
constexpr float RND_ALPHA_MAX = 0.99f, RND_ALPHA_MIN = 1.0f / 255.0f, RND_T_MIN = 1e-4f;
enum { RND_ST_VISIBLE = 0, RND_ST_WORDS = 4 };

constexpr double SH_C0 = 0.28209479177387814, SH_C1 = 0.4886025119029199;
__device__ const double SH_C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
__device__ const double SH_C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                                    1.445305721320277, -0.5900435899266435};

struct RndWs {
    uint4 *rec;                                  // n records of four quads
    unsigned long long *counts, *offsets;        // n + 1 each: tiles per row | its first instance; offsets[n] = all instances
    uint2 *ranges;                               // tile -> [first, last + 1) of its sorted instances
    unsigned *state;
    void *temp;
    size_t temp_bytes, total;
};

struct RndInst {
    unsigned long long *keys0, *keys1;
    unsigned *rows0, *rows1;
    void *temp;
    size_t temp_bytes, total;
};

static size_t rnd_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int rnd_tiles(int side) { return (side + RND_TILE - 1) / RND_TILE; }

static int rnd_carve(int64_t n, int width, int height, void *base, hipStream_t stream, RndWs *w)
{
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    size_t t_scan = 0;
    unsigned long long *v = nullptr;
    if (rocprim::exclusive_scan(nullptr, t_scan, v, v, 0ull, m + 1, rocprim::plus<unsigned long long>(), stream) != hipSuccess)
        GSX_FAIL("gsx_rows_render: rocprim size query failed");
    w->temp_bytes = t_scan;
    char *p = static_cast<char *>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + at : nullptr;
        at += rnd_align(bytes);
        return q;
    };
    w->rec = reinterpret_cast<uint4 *>(take(4 * GSX_RENDER_RECORD_WORDS * m));
    w->counts = reinterpret_cast<unsigned long long *>(take(8 * (m + 1)));
    w->offsets = reinterpret_cast<unsigned long long *>(take(8 * (m + 1)));
    w->ranges = reinterpret_cast<uint2 *>(take(8 * (size_t)rnd_tiles(width) * rnd_tiles(height)));
    w->state = reinterpret_cast<unsigned *>(take(4 * RND_ST_WORDS));
    w->temp = take(w->temp_bytes);
    w->total = at;
    return 0;
}

// bits of the sort: the depth's 32 and what the tile index needs
static int rnd_key_bits(int width, int height)
{
    const unsigned tiles = (unsigned)(rnd_tiles(width) * rnd_tiles(height));
    int bits = 1;
    while ((1u << bits) < tiles) ++bits;
    return 32 + bits;
}

static int rnd_carve_inst(int64_t total, int key_bits, void *base, hipStream_t stream, RndInst *w)
{
    const size_t m = (size_t)std::max<int64_t>(total, 1);
    size_t t_sort = 0;
    unsigned long long *k = nullptr;
    unsigned *v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, t_sort, k, k, v, v, m, 0, key_bits, stream) != hipSuccess)
        GSX_FAIL("gsx_rows_render: rocprim size query failed");
    w->temp_bytes = t_sort;
    char *p = static_cast<char *>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + at : nullptr;
        at += rnd_align(bytes);
        return q;
    };
    w->keys0 = reinterpret_cast<unsigned long long *>(take(8 * m));
    w->keys1 = reinterpret_cast<unsigned long long *>(take(8 * m));
    w->rows0 = reinterpret_cast<unsigned *>(take(4 * m));
    w->rows1 = reinterpret_cast<unsigned *>(take(4 * m));
    w->temp = take(w->temp_bytes);
    w->total = at;
    return 0;
}

// ---- (a) project

struct RndRecord {
    float u, v, a, b, c, opac, col[3], depth;
    int x0, x1, y0, y1;
};

__device__ __forceinline__ bool rnd_finite(float v) { return fabsf(v) < __builtin_inff(); }

// the colour of the row at byte `rb` before its rounding to float32: the SH bands up to L.degree along normalize(p - eye), + 0.5,
// values not above 0 become 0; or byte / 255
__device__ __forceinline__ void rnd_colour(const unsigned char *__restrict__ rows, int64_t rb, const gsx_render_layout &L, double px, double py,
                                           double pz, float *col)
{
    if (L.dc_offset[0] < 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)                                      // (rgb_offset[0] < 0: a scoring plan reads no colour)
            col[ch] = L.rgb_offset[0] < 0 ? 0.0f : __double2float_rn(__ddiv_rn((double)rows[rb + L.rgb_offset[ch]], 255.0));
        return;
    }
    double Y[16];
    Y[0] = SH_C0;
    if (L.degree >= 1) {
        const double dx = px - L.eye[0], dy = py - L.eye[1], dz = pz - L.eye[2];
        const double nn = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
        const double x = __ddiv_rn(dx, nn), y = __ddiv_rn(dy, nn), z = __ddiv_rn(dz, nn);
        Y[1] = (-SH_C1) * y;
        Y[2] = SH_C1 * z;
        Y[3] = (-SH_C1) * x;
        if (L.degree >= 2) {
            const double xx = x * x, yy = y * y, zz = z * z;
            Y[4] = (SH_C2[0] * x) * y;
            Y[5] = (SH_C2[1] * y) * z;
            Y[6] = SH_C2[2] * ((2.0 * zz - xx) - yy);
            Y[7] = (SH_C2[3] * x) * z;
            Y[8] = SH_C2[4] * (xx - yy);
            if (L.degree >= 3) {
                Y[9] = (SH_C3[0] * y) * (3.0 * xx - yy);
                Y[10] = ((SH_C3[1] * x) * y) * z;
                Y[11] = (SH_C3[2] * y) * ((4.0 * zz - xx) - yy);
                Y[12] = (SH_C3[3] * z) * ((2.0 * zz - 3.0 * xx) - 3.0 * yy);
                Y[13] = (SH_C3[4] * x) * ((4.0 * zz - xx) - yy);
                Y[14] = (SH_C3[5] * z) * (xx - yy);
                Y[15] = (SH_C3[6] * x) * (xx - 3.0 * yy);
            }
        }
    }
    const int used = (L.degree + 1) * (L.degree + 1);
    for (int ch = 0; ch < 3; ++ch) {
        double res = SH_C0 * (double)ld_f32(rows, rb + L.dc_offset[ch]);
        for (int k = 1; k < used; ++k) res = res + Y[k] * (double)ld_f32(rows, rb + L.rest_offset[ch * L.rest_m + k - 1]);
        res = res + 0.5;
        col[ch] = __double2float_rn(res > 0.0 ? res : 0.0);
    }
}

// the definition's record of the row at byte `rb`; false: the row is invisible
__device__ __forceinline__ bool rnd_project_row(const unsigned char *__restrict__ rows, int64_t rb, const gsx_render_layout &L, RndRecord *r)
{
    const float fx_ = ld_f32(rows, rb + L.xyz_offset[0]), fy_ = ld_f32(rows, rb + L.xyz_offset[1]), fz_ = ld_f32(rows, rb + L.xyz_offset[2]);
    const float s0 = ld_f32(rows, rb + L.scale_offset[0]), s1 = ld_f32(rows, rb + L.scale_offset[1]), s2 = ld_f32(rows, rb + L.scale_offset[2]);
    const float r0 = ld_f32(rows, rb + L.rot_offset[0]), r1 = ld_f32(rows, rb + L.rot_offset[1]), r2 = ld_f32(rows, rb + L.rot_offset[2]),
                r3 = ld_f32(rows, rb + L.rot_offset[3]);
    const float op = ld_f32(rows, rb + L.opacity_offset);
    if (!(rnd_finite(fx_) && rnd_finite(fy_) && rnd_finite(fz_) && rnd_finite(s0) && rnd_finite(s1) && rnd_finite(s2) && rnd_finite(r0) &&
          rnd_finite(r1) && rnd_finite(r2) && rnd_finite(r3) && rnd_finite(op)))
        return false;
    const double x = (double)fx_, y = (double)fy_, z = (double)fz_;
    const double *V = L.view;
    const double xc = ((V[0] * x + V[1] * y) + V[2] * z) + V[3];
    const double yc = ((V[4] * x + V[5] * y) + V[6] * z) + V[7];
    const double zc = ((V[8] * x + V[9] * y) + V[10] * z) + V[11];
    if (!(zc > L.near)) return false;
    const double a0 = (double)r0, a1 = (double)r1, a2 = (double)r2, a3 = (double)r3;
    const double qq = ((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3;
    if (!(qq > 0.0)) return false;
    const double nn = __dsqrt_rn(qq);
    const double qw = __ddiv_rn(a0, nn), qx = __ddiv_rn(a1, nn), qy = __ddiv_rn(a2, nn), qz = __ddiv_rn(a3, nn);
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const double xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const double wx = qw * qx, wy = qw * qy, wz = qw * qz;
    const double R[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                            {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                            {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
    const double e0 = (double)np_expf(s0), e1 = (double)np_expf(s1), e2 = (double)np_expf(s2);
    const double v0 = e0 * e0, v1 = e1 * e1, v2 = e2 * e2;
    double S[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) S[j][k] = ((R[j][0] * v0) * R[k][0] + (R[j][1] * v1) * R[k][1]) + (R[j][2] * v2) * R[k][2];
    const double limx = 1.3 * L.tan_fovx, limy = 1.3 * L.tan_fovy;
    const double xzr = __ddiv_rn(xc, zc), yzr = __ddiv_rn(yc, zc);
    const double tx = fmin(limx, fmax(-limx, xzr)) * zc, ty = fmin(limy, fmax(-limy, yzr)) * zc;
    const double z2 = zc * zc;
    const double j00 = __ddiv_rn(L.fx, zc), j02 = __ddiv_rn(-(L.fx * tx), z2);
    const double j11 = __ddiv_rn(L.fy, zc), j12 = __ddiv_rn(-(L.fy * ty), z2);
    double T[2][3], M[2][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T[0][k] = j00 * V[k] + j02 * V[8 + k];
        T[1][k] = j11 * V[4 + k] + j12 * V[8 + k];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[q][k] = (T[q][0] * S[0][k] + T[q][1] * S[1][k]) + T[q][2] * S[2][k];
    const double sxx = ((M[0][0] * T[0][0] + M[0][1] * T[0][1]) + M[0][2] * T[0][2]) + 0.3;
    const double sxy = (M[0][0] * T[1][0] + M[0][1] * T[1][1]) + M[0][2] * T[1][2];
    const double syy = ((M[1][0] * T[1][0] + M[1][1] * T[1][1]) + M[1][2] * T[1][2]) + 0.3;
    const double det = sxx * syy - sxy * sxy;
    if (!(det > 0.0 && det < (double)__builtin_inff())) return false;
    const double mid = 0.5 * (sxx + syy);
    const double disc = mid * mid - det;
    const double rad = ceil(3.0 * __dsqrt_rn(mid + __dsqrt_rn(disc > 0.1 ? disc : 0.1)));
    const double u = L.fx * xzr + L.cx, v = L.fy * yzr + L.cy;
    const double x0 = fmax(ceil(u - rad), 0.0), x1 = fmin(floor(u + rad), (double)L.width - 1.0);
    const double y0 = fmax(ceil(v - rad), 0.0), y1 = fmin(floor(v + rad), (double)L.height - 1.0);
    if (!(x0 <= x1 && y0 <= y1)) return false;
    r->u = __double2float_rn(u);
    r->v = __double2float_rn(v);
    r->a = __double2float_rn(__ddiv_rn(syy, det));
    r->b = __double2float_rn(__ddiv_rn(-sxy, det));
    r->c = __double2float_rn(__ddiv_rn(sxx, det));
    r->opac = __fdiv_rn(1.0f, __fadd_rn(1.0f, np_expf(-op)));     // splat_metric.h's expression
    r->depth = __double2float_rn(zc);
    r->x0 = (int)x0;
    r->x1 = (int)x1;
    r->y0 = (int)y0;
    r->y1 = (int)y1;
    rnd_colour(rows, rb, L, x, y, z, r->col);
    return true;
}

__global__ __launch_bounds__(256) void rnd_project_kernel(const unsigned char *__restrict__ rows, int64_t first, int64_t stride, int64_t n,
                                                          gsx_render_layout L, uint4 *__restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    RndRecord r;
    uint4 q[RND_QUADS] = {};
    if (rnd_project_row(rows, first + i * stride, L, &r)) {
        q[0] = make_uint4(__float_as_uint(r.u), __float_as_uint(r.v), __float_as_uint(r.a), __float_as_uint(r.b));
        q[1] = make_uint4(__float_as_uint(r.c), __float_as_uint(r.opac), __float_as_uint(r.col[0]), __float_as_uint(r.col[1]));
        q[2] = make_uint4(__float_as_uint(r.col[2]), __float_as_uint(r.depth), (unsigned)r.x0, (unsigned)r.x1);
        q[3] = make_uint4((unsigned)r.y0, (unsigned)r.y1, 1u, 0u);
    }
#pragma unroll
    for (int k = 0; k < RND_QUADS; ++k) rec[i * RND_QUADS + k] = q[k];
}

// ---- (b) count: tiles per row; entry n is the scan's closing zero

__global__ __launch_bounds__(256) void rnd_count_kernel(const uint4 *__restrict__ rec, int64_t n, unsigned long long *__restrict__ counts,
                                                        unsigned *__restrict__ state)
{
    // grid-stride: a wave adds its visible rows up and sends one atomic (one per wave and row block took longer than the scan)
    unsigned seen = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (int64_t)gridDim.x * 256) {
        unsigned long long cnt = 0;
        if (i < n) {
            const uint4 q2 = rec[i * RND_QUADS + 2], q3 = rec[i * RND_QUADS + 3];
            if (q3.z != 0u) {
                ++seen;
                cnt = (unsigned long long)((q2.w / RND_TILE) - (q2.z / RND_TILE) + 1u) * (unsigned long long)((q3.y / RND_TILE) - (q3.x / RND_TILE) + 1u);
            }
        }
        counts[i] = cnt;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) seen += __shfl_down(seen, d, 64);    // (a count: integer adds, the same whatever their order)
    if ((threadIdx.x & 63) == 0 && seen) atomicAdd(&state[RND_ST_VISIBLE], seen);
}

// ---- (c) emit

__global__ __launch_bounds__(256) void rnd_emit_kernel(const uint4 *__restrict__ rec, const unsigned long long *__restrict__ offsets, int64_t n,
                                                       int tiles_x, unsigned long long *__restrict__ keys, unsigned *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 q3 = rec[i * RND_QUADS + 3];
    if (q3.z == 0u) return;
    const uint4 q2 = rec[i * RND_QUADS + 2];
    const unsigned tx0 = q2.z / RND_TILE, tx1 = q2.w / RND_TILE, ty0 = q3.x / RND_TILE, ty1 = q3.y / RND_TILE;
    unsigned long long o = offsets[i];
    for (unsigned ty = ty0; ty <= ty1; ++ty)
        for (unsigned tx = tx0; tx <= tx1; ++tx) {
            keys[o] = ((unsigned long long)(ty * (unsigned)tiles_x + tx) << 32) | q2.y;     // q2.y: the depth's bits, a float above 0
            vals[o] = (unsigned)i;
            ++o;
        }
}

// ---- (e) tile ranges

__global__ __launch_bounds__(256) void rnd_ranges_kernel(const unsigned long long *__restrict__ ks, int64_t total, uint2 *__restrict__ ranges)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const unsigned tile = (unsigned)(ks[p] >> 32);
    if (p == 0 || (unsigned)(ks[p - 1] >> 32) != tile) ranges[tile].x = (unsigned)p;
    if (p == total - 1 || (unsigned)(ks[p + 1] >> 32) != tile) ranges[tile].y = (unsigned)(p + 1);
}

// ---- (f) blend

__device__ __forceinline__ unsigned char rnd_byte(float colour, float T, float bg)
{
    float o = __fadd_rn(colour, __fmul_rn(T, bg));
    o = o < 0.0f ? 0.0f : (o > 1.0f ? 1.0f : o);
    return (unsigned char)(int)floorf(__fadd_rn(__fmul_rn(o, 255.0f), 0.5f));
}

__global__ __launch_bounds__(256) void rnd_blend_kernel(const uint4 *__restrict__ rec, const unsigned *__restrict__ srows,
                                                        const uint2 *__restrict__ ranges, int width, int height, int tiles_x, float bg0, float bg1,
                                                        float bg2, unsigned char *__restrict__ image)
{
    __shared__ uint4 s_rec[RND_BATCH * RND_QUADS];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int px = (tile % tiles_x) * RND_TILE + (t & (RND_TILE - 1)), py = (tile / tiles_x) * RND_TILE + t / RND_TILE;
    const bool inside = px < width && py < height;
    const float fpx = (float)px, fpy = (float)py;
    float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    bool done = !inside;
    const uint2 rg = ranges[tile];
    for (unsigned base = rg.x; base < rg.y; base += RND_BATCH) {
        if (__syncthreads_and(done)) break;               // (also: the last batch's readers have left s_rec)
        const int cnt = (int)min((unsigned)RND_BATCH, rg.y - base);
        for (int q = t; q < cnt * RND_QUADS; q += 256) s_rec[q] = rec[(size_t)srows[base + (unsigned)(q / RND_QUADS)] * RND_QUADS + (q % RND_QUADS)];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            if (__ballot(!done) == 0ull) break;           // this wave's strip is finished
            if (done) continue;
            const uint4 q2 = s_rec[j * RND_QUADS + 2], q3 = s_rec[j * RND_QUADS + 3];
            if (px < (int)q2.z || px > (int)q2.w || py < (int)q3.x || py > (int)q3.y) continue;
            const uint4 q0 = s_rec[j * RND_QUADS], q1 = s_rec[j * RND_QUADS + 1];
            const float dx = __fsub_rn(__uint_as_float(q0.x), fpx), dy = __fsub_rn(__uint_as_float(q0.y), fpy);
            const float a = __uint_as_float(q0.z), b = __uint_as_float(q0.w), c = __uint_as_float(q1.x);
            const float power = __fsub_rn(__fmul_rn(-0.5f, __fadd_rn(__fmul_rn(a, __fmul_rn(dx, dx)), __fmul_rn(c, __fmul_rn(dy, dy)))),
                                          __fmul_rn(__fmul_rn(b, dx), dy));
            if (!(power <= 0.0f) || power < RND_POWER_CUT) continue;
            const float alpha = fminf(RND_ALPHA_MAX, __fmul_rn(__uint_as_float(q1.y), np_expf(power)));
            if (alpha < RND_ALPHA_MIN) continue;
            const float Tn = __fmul_rn(T, __fsub_rn(1.0f, alpha));
            if (Tn < RND_T_MIN) {
                done = true;
                continue;
            }
            const float wgt = __fmul_rn(alpha, T);
            c0 = __fadd_rn(c0, __fmul_rn(__uint_as_float(q1.z), wgt));
            c1 = __fadd_rn(c1, __fmul_rn(__uint_as_float(q1.w), wgt));
            c2 = __fadd_rn(c2, __fmul_rn(__uint_as_float(q2.x), wgt));
            T = Tn;
        }
    }
    if (inside) {
        unsigned char *o = image + ((size_t)py * width + px) * 3;
        o[0] = rnd_byte(c0, T, bg0);
        o[1] = rnd_byte(c1, T, bg1);
        o[2] = rnd_byte(c2, T, bg2);
    }
}

// ---- (g) score

constexpr float RND_SCORE_UNIT = 16777216.0f;    // 2^24: a weight in [3.9e-7, 0.99] times it truncates to an integer below 2^24

__global__ __launch_bounds__(256) void rnd_score_kernel(const uint4 *__restrict__ rec, const unsigned *__restrict__ srows,
                                                        const uint2 *__restrict__ ranges, int width, int height, int tiles_x,
                                                        unsigned *__restrict__ peak, unsigned long long *__restrict__ total)
{
    __shared__ uint4 s_rec[RND_BATCH * RND_QUADS];
    __shared__ unsigned s_peak[RND_BATCH], s_sum[RND_BATCH];     // per record of the batch: max of the float bits | sum, < 256 * 2^24
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int px = (tile % tiles_x) * RND_TILE + (t & (RND_TILE - 1)), py = (tile / tiles_x) * RND_TILE + t / RND_TILE;
    const float fpx = (float)px, fpy = (float)py;
    float T = 1.0f;
    bool done = !(px < width && py < height);
    s_peak[t] = 0u;
    s_sum[t] = 0u;
    const uint2 rg = ranges[tile];
    for (unsigned base = rg.x; base < rg.y; base += RND_BATCH) {
        if (__syncthreads_and(done)) break;               // (also: the last batch's readers have left s_rec)
        const int cnt = (int)min((unsigned)RND_BATCH, rg.y - base);
        for (int q = t; q < cnt * RND_QUADS; q += 256) s_rec[q] = rec[(size_t)srows[base + (unsigned)(q / RND_QUADS)] * RND_QUADS + (q % RND_QUADS)];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            if (__ballot(!done) == 0ull) break;           // this wave's strip is finished
            float wgt = 0.0f;                             // (a weight that is added is >= 1/255 * 1e-4 > 0)
            if (!done) {
                const uint4 q2 = s_rec[j * RND_QUADS + 2], q3 = s_rec[j * RND_QUADS + 3];
                if (!(px < (int)q2.z || px > (int)q2.w || py < (int)q3.x || py > (int)q3.y)) {
                    const uint4 q0 = s_rec[j * RND_QUADS], q1 = s_rec[j * RND_QUADS + 1];
                    const float dx = __fsub_rn(__uint_as_float(q0.x), fpx), dy = __fsub_rn(__uint_as_float(q0.y), fpy);
                    const float a = __uint_as_float(q0.z), b = __uint_as_float(q0.w), c = __uint_as_float(q1.x);
                    const float power = __fsub_rn(__fmul_rn(-0.5f, __fadd_rn(__fmul_rn(a, __fmul_rn(dx, dx)), __fmul_rn(c, __fmul_rn(dy, dy)))),
                                                  __fmul_rn(__fmul_rn(b, dx), dy));
                    if (power <= 0.0f && !(power < RND_POWER_CUT)) {
                        const float alpha = fminf(RND_ALPHA_MAX, __fmul_rn(__uint_as_float(q1.y), np_expf(power)));
                        if (!(alpha < RND_ALPHA_MIN)) {
                            const float Tn = __fmul_rn(T, __fsub_rn(1.0f, alpha));
                            if (Tn < RND_T_MIN) {
                                done = true;
                            } else {
                                wgt = __fmul_rn(alpha, T);
                                T = Tn;
                            }
                        }
                    }
                }
            }
            if (__ballot(wgt > 0.0f) == 0ull) continue;  // most records miss most strips
            unsigned mx = __float_as_uint(wgt), sum = (unsigned)__fmul_rn(wgt, RND_SCORE_UNIT);     // 64 sums below 2^24: below 2^30
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                mx = max(mx, (unsigned)__shfl_xor((int)mx, d, 64));
                sum += (unsigned)__shfl_xor((int)sum, d, 64);
            }
            if ((t & 63) == 0) {
                atomicMax(&s_peak[j], mx);
                atomicAdd(&s_sum[j], sum);
            }
        }
        __syncthreads();
        // lane t owns record t of the batch: it sends the words on and clears them for the next batch
        const unsigned sum = s_sum[t];
        if (sum) {                                        // (t < cnt: no wave wrote a word at or above cnt)
            const unsigned row = srows[base + (unsigned)t];
            atomicMax(&peak[row], s_peak[t]);
            atomicAdd(&total[row], (unsigned long long)sum);
            s_peak[t] = 0u;
            s_sum[t] = 0u;
        }
    }
}

__global__ __launch_bounds__(256) void view_keys_kernel(const unsigned long long *__restrict__ total, int64_t n, unsigned *__restrict__ keys)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) keys[i] = view_key_of(total[i]);
}

// the layout's refusals: every field inside a row, a degree the coefficients cover, an image and a camera the kernels can use
static int rnd_check_layout(const gsx_render_layout *l, int64_t stride, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (l->width < 1 || l->width > GSX_RENDER_MAX_SIDE || l->height < 1 || l->height > GSX_RENDER_MAX_SIDE)
        GSX_FAIL("%s: an image of %d x %d (1 ... %d per side)", who, l->width, l->height, GSX_RENDER_MAX_SIDE);
    if (stride == 0) return 0;                   // (the draw call: the rows are not read again)
    auto inside = [&](int o, int bytes, const char *what, int k) -> int {
        if (o < 0 || o + bytes > stride) GSX_FAIL("%s: %s field %d at byte offset %d of a %lld-byte row", who, what, k, o, (long long)stride);
        return 0;
    };
    for (int a = 0; a < 3; ++a) {
        GSX_CHECK(inside(l->xyz_offset[a], 4, "position", a));
        GSX_CHECK(inside(l->scale_offset[a], 4, "scale", a));
    }
    for (int a = 0; a < 4; ++a) GSX_CHECK(inside(l->rot_offset[a], 4, "rotation", a));
    GSX_CHECK(inside(l->opacity_offset, 4, "opacity", 0));
    if (l->dc_offset[0] < 0) {
        for (int a = 0; a < 3 && l->rgb_offset[0] >= 0; ++a) GSX_CHECK(inside(l->rgb_offset[a], 1, "colour", a));
    } else {
        const int used = (l->degree + 1) * (l->degree + 1) - 1;
        if (l->degree < 0 || l->degree > 3 || (l->rest_m != 0 && l->rest_m != 3 && l->rest_m != 8 && l->rest_m != 15) || used > l->rest_m)
            GSX_FAIL("%s: SH degree %d with %d f_rest coefficients per channel (0, 3, 8 or 15; degree 0 ... 3)", who, l->degree, l->rest_m);
        for (int a = 0; a < 3; ++a) GSX_CHECK(inside(l->dc_offset[a], 4, "f_dc", a));
        for (int ch = 0; ch < 3; ++ch)
            for (int k = 0; k < used; ++k) GSX_CHECK(inside(l->rest_offset[ch * l->rest_m + k], 4, "f_rest", ch * l->rest_m + k));
    }
    bool finite = l->near > 0.0 && l->near < (double)__builtin_inff() && l->tan_fovx > 0.0 && l->tan_fovy > 0.0;
    const double nums[6] = {l->fx, l->fy, l->cx, l->cy, l->tan_fovx, l->tan_fovy};
    for (double v : nums) finite = finite && fabs(v) < (double)__builtin_inff();
    for (double v : l->view) finite = finite && fabs(v) < (double)__builtin_inff();
    for (double v : l->eye) finite = finite && fabs(v) < (double)__builtin_inff();
    if (!finite) GSX_FAIL("%s: the camera's numbers must be finite, near and the field of view above 0", who);
    return 0;
}

// stream clocks of consecutive stages: mark() after each, read() joins the stream and adds the milliseconds between the marks
struct RndClock {
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int used = 0;
    bool on;
    hipStream_t stream;
    RndClock(bool on_, hipStream_t s) : on(on_), stream(s) {}
    ~RndClock()
    {
        for (int k = 0; k < 5; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
    int mark()
    {
        if (!on) return 0;
        GSX_HIP(hipEventCreate(&ev[used]));
        GSX_HIP(hipEventRecord(ev[used], stream));
        ++used;
        return 0;
    }
    int read(float *into)
    {
        if (!on) return 0;
        GSX_HIP(hipStreamSynchronize(stream));
        for (int k = 0; k + 1 < used; ++k) {
            float ms = 0.0f;
            GSX_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            into[k] += ms;
        }
        return 0;
    }
};

static int rnd_common(gsx_ctx *c, int64_t n, const void *work_dev, const char *who)
{
    if (!c || !work_dev) GSX_FAIL("%s: null argument", who);
    if (n < 0 || n >= (1LL << 31)) GSX_FAIL("%s: %lld rows (fewer than 2^31)", who, (long long)n);
    if (reinterpret_cast<uintptr_t>(work_dev) & 15) GSX_FAIL("%s: the workspace must be 16-byte aligned", who);
    return 0;
}

// (c) (d) (e) of a plan, for the draw call and the score call alike: the plan's own total read again, the instance workspace
// carved, emit, the stable sort and the tile ranges, with the clock's marks before emit and after each -> the workspace, the
// sorted rows (null without instances) and the total
static int rnd_order(gsx_ctx *c, int64_t n, const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, void *inst_dev, int64_t inst_bytes,
                     const char *who, RndClock *clock, RndWs *w, const unsigned **sorted_rows, unsigned long long *total_out)
{
    GSX_CHECK(rnd_check_layout(layout, 0, who));
    if (reinterpret_cast<uintptr_t>(inst_dev) & 15) GSX_FAIL("%s: the instance workspace must be 16-byte aligned", who);
    GSX_HIP(hipSetDevice(c->device));
    const int width = layout->width, height = layout->height, tiles_x = rnd_tiles(width), tiles = tiles_x * rnd_tiles(height);
    GSX_CHECK(rnd_carve(n, width, height, work_dev, c->stream, w));
    if ((int64_t)w->total > work_bytes) GSX_FAIL("%s: a workspace of %lld bytes, %zu are needed", who, (long long)work_bytes, w->total);
    // the plan's own total, read again: the launches below are sized by it, not by the caller's word
    unsigned long long total = 0;
    if (n > 0) {
        GSX_HIP(hipMemcpyAsync(&total, w->offsets + n, 8, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(hipStreamSynchronize(c->stream));
    }
    if (total >= (1ull << 31)) GSX_FAIL("%s: %llu instances (fewer than 2^31)", who, total);
    RndInst inst = {};
    if (total) {
        GSX_CHECK(rnd_carve_inst((int64_t)total, rnd_key_bits(width, height), inst_dev, c->stream, &inst));
        if (!inst_dev || (int64_t)inst.total > inst_bytes)
            GSX_FAIL("%s: an instance workspace of %lld bytes, %zu are needed", who, (long long)(inst_dev ? inst_bytes : 0), inst.total);
    }
    GSX_HIP(hipMemsetAsync(w->ranges, 0, 8 * (size_t)tiles, c->stream));
    GSX_CHECK(clock->mark());
    *sorted_rows = nullptr;
    if (total) {
        hipLaunchKernelGGL(rnd_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, w->rec, w->offsets, n, tiles_x, inst.keys0, inst.rows0);
        GSX_HIP(hipGetLastError());
    }
    GSX_CHECK(clock->mark());
    if (total) {
        size_t tb = inst.temp_bytes;
        GSX_HIP(rocprim::radix_sort_pairs(inst.temp, tb, inst.keys0, inst.keys1, inst.rows0, inst.rows1, (size_t)total, 0, rnd_key_bits(width, height),
                                          c->stream));                                                                    // stable
        *sorted_rows = inst.rows1;
    }
    GSX_CHECK(clock->mark());
    if (total) {
        hipLaunchKernelGGL(rnd_ranges_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, inst.keys1, (int64_t)total, w->ranges);
        GSX_HIP(hipGetLastError());
    }
    GSX_CHECK(clock->mark());
    *total_out = total;
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_rows_render_work_dev(gsx_ctx *c, int64_t n, int32_t width, int32_t height, int64_t *bytes_out)
{
    const char *who = "gsx_rows_render_work_dev";
    if (!c || !bytes_out) GSX_FAIL("%s: null argument", who);
    if (n < 0 || n >= (1LL << 31)) GSX_FAIL("%s: %lld rows (fewer than 2^31)", who, (long long)n);
    if (width < 1 || width > GSX_RENDER_MAX_SIDE || height < 1 || height > GSX_RENDER_MAX_SIDE)
        GSX_FAIL("%s: an image of %d x %d (1 ... %d per side)", who, width, height, GSX_RENDER_MAX_SIDE);
    GSX_HIP(hipSetDevice(c->device));
    RndWs w;
    GSX_CHECK(rnd_carve(n, width, height, nullptr, c->stream, &w));
    *bytes_out = (int64_t)w.total;
    return 0;
}

int gsx_rows_render_plan_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n, const gsx_render_layout *layout,
                             void *work_dev, int64_t work_bytes, int64_t *info_out, float *stage_ms)
{
    const char *who = "gsx_rows_render_plan_dev";
    if (!info_out) GSX_FAIL("%s: null argument", who);
    GSX_CHECK(rnd_common(c, n, work_dev, who));
    if (n > 0 && !rows_dev) GSX_FAIL("%s: null argument", who);
    GSX_CHECK(rows_args(rows_dev, first_byte, stride, who));
    GSX_CHECK(rnd_check_layout(layout, stride, who));
    for (int k = 0; k < GSX_RENDER_INFO_WORDS; ++k) info_out[k] = 0;
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    RndWs w;
    GSX_CHECK(rnd_carve(n, layout->width, layout->height, work_dev, c->stream, &w));
    if ((int64_t)w.total > work_bytes) GSX_FAIL("%s: a workspace of %lld bytes, %zu are needed", who, (long long)work_bytes, w.total);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    RndClock clock(stage_ms != nullptr, c->stream);
    GSX_HIP(hipMemsetAsync(w.state, 0, 4 * RND_ST_WORDS, c->stream));
    GSX_CHECK(clock.mark());
    hipLaunchKernelGGL(rnd_project_kernel, dim3(blocks), dim3(256), 0, c->stream, static_cast<const unsigned char *>(rows_dev), first_byte, stride, n,
                       *layout, w.rec);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(clock.mark());
    hipLaunchKernelGGL(rnd_count_kernel, dim3(tile_blocks(c, n + 1, 256, 8)), dim3(256), 0, c->stream, w.rec, n, w.counts, w.state);
    GSX_HIP(hipGetLastError());
    size_t tb = w.temp_bytes;
    GSX_HIP(rocprim::exclusive_scan(w.temp, tb, w.counts, w.offsets, 0ull, (size_t)n + 1, rocprim::plus<unsigned long long>(), c->stream));
    GSX_CHECK(clock.mark());
    unsigned state[RND_ST_WORDS] = {0, 0, 0, 0};
    unsigned long long total = 0;
    GSX_HIP(hipMemcpyAsync(state, w.state, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipMemcpyAsync(&total, w.offsets + n, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if (stage_ms) GSX_CHECK(clock.read(stage_ms));
    info_out[1] = state[RND_ST_VISIBLE];
    info_out[2] = (int64_t)std::min<unsigned long long>(total, (unsigned long long)INT64_MAX);
    if (total >= (1ull << 31)) {
        info_out[0] = GSX_RENDER_TOO_MANY;
        info_out[3] = (int64_t)std::min<unsigned long long>(total, (unsigned long long)(INT64_MAX / 32)) * 24;   // the four arrays; a lower bound
        return 0;
    }
    RndInst inst;
    GSX_CHECK(rnd_carve_inst((int64_t)total, rnd_key_bits(layout->width, layout->height), nullptr, c->stream, &inst));
    info_out[3] = total ? (int64_t)inst.total : 0;
    return 0;
}

int gsx_rows_render_draw_dev(gsx_ctx *c, int64_t n, const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, void *inst_dev,
                             int64_t inst_bytes, void *image_dev, float *stage_ms)
{
    const char *who = "gsx_rows_render_draw_dev";
    GSX_CHECK(rnd_common(c, n, work_dev, who));
    if (!image_dev) GSX_FAIL("%s: null argument", who);
    RndWs w;
    RndClock clock(stage_ms != nullptr, c->stream);
    const unsigned *sorted_rows = nullptr;
    unsigned long long total = 0;
    GSX_CHECK(rnd_order(c, n, layout, work_dev, work_bytes, inst_dev, inst_bytes, who, &clock, &w, &sorted_rows, &total));
    const int tiles_x = rnd_tiles(layout->width), tiles = tiles_x * rnd_tiles(layout->height);
    hipLaunchKernelGGL(rnd_blend_kernel, dim3((unsigned)tiles), dim3(256), 0, c->stream, w.rec, sorted_rows, w.ranges, layout->width, layout->height,
                       tiles_x, layout->background[0], layout->background[1], layout->background[2], static_cast<unsigned char *>(image_dev));
    GSX_HIP(hipGetLastError());
    GSX_CHECK(clock.mark());
    if (stage_ms) GSX_CHECK(clock.read(stage_ms + 2));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_rows_render_score_dev(gsx_ctx *c, int64_t n, const gsx_render_layout *layout, void *work_dev, int64_t work_bytes, void *inst_dev,
                              int64_t inst_bytes, uint32_t *peak_dev, uint64_t *total_dev, float *stage_ms)
{
    const char *who = "gsx_rows_render_score_dev";
    GSX_CHECK(rnd_common(c, n, work_dev, who));
    if (n > 0 && (!peak_dev || !total_dev)) GSX_FAIL("%s: null argument", who);
    if ((reinterpret_cast<uintptr_t>(peak_dev) & 3) || (reinterpret_cast<uintptr_t>(total_dev) & 7))
        GSX_FAIL("%s: the peaks must be 4-byte aligned, the totals 8-byte aligned", who);
    RndWs w;
    RndClock clock(stage_ms != nullptr, c->stream);
    const unsigned *sorted_rows = nullptr;
    unsigned long long total = 0;
    GSX_CHECK(rnd_order(c, n, layout, work_dev, work_bytes, inst_dev, inst_bytes, who, &clock, &w, &sorted_rows, &total));
    if (total) {                                 // (no instance: no row is blended, nothing to add)
        const int tiles_x = rnd_tiles(layout->width), tiles = tiles_x * rnd_tiles(layout->height);
        hipLaunchKernelGGL(rnd_score_kernel, dim3((unsigned)tiles), dim3(256), 0, c->stream, w.rec, sorted_rows, w.ranges, layout->width,
                           layout->height, tiles_x, peak_dev, reinterpret_cast<unsigned long long *>(total_dev));
        GSX_HIP(hipGetLastError());
    }
    GSX_CHECK(clock.mark());
    if (stage_ms) GSX_CHECK(clock.read(stage_ms + 2));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_view_keys_dev(gsx_ctx *c, const uint64_t *total_dev, int64_t n, uint32_t *keys_dev)
{
    if (!c || (n > 0 && (!total_dev || !keys_dev))) GSX_FAIL("gsx_view_keys_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_view_keys_dev: 0 <= n < 2^32");
    if ((reinterpret_cast<uintptr_t>(total_dev) & 7) || (reinterpret_cast<uintptr_t>(keys_dev) & 3))
        GSX_FAIL("gsx_view_keys_dev: the totals must be 8-byte aligned, the keys 4-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(view_keys_kernel, dim3(tile_blocks(c, n, 1024, 8)), dim3(256), 0, c->stream,
                       reinterpret_cast<const unsigned long long *>(total_dev), n, keys_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_view_keys_host(const uint64_t *total, int64_t n, uint32_t *keys)
{
    if (n > 0 && (!total || !keys)) GSX_FAIL("gsx_view_keys_host: null argument");
    if (n < 0) GSX_FAIL("gsx_view_keys_host: n >= 0");
    for (int64_t i = 0; i < n; ++i) keys[i] = view_key_of(total[i]);
    return 0;
}

}  // extern "C"
