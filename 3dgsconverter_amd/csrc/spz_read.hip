// spz_read.hip -- the SPZ reader's decode: the six planar sections of an inflated .spz body -> the reference's rows
// (GaussianStruct.define_dtype(has_rgb=True)), bit for bit.
//
// Replaces, in gsconverter/formats/spz.py (SpzFormat._read_body):
//   positions     :182-197  version 1: float16 -> float32 (numpy's cast: a signalling NaN stays signalling); else the
//                           sign-extended 24-bit integer as float32, divided by float32(1 << fractional_bits) (inf from 128 bits
//                           on: +-0 with the integer's sign; subnormal quotients are kept)
//   opacity       :200, :345-348  a 256-entry float32 table the host builds with numpy (no device log)
//   colour        :204-216  two 256-entry tables: f_dc, and the red/green/blue byte the reference derives from it
//   scale         :219-222  b / 16 - 10: exact in float32 as in the reference's float64, so computed
//   rotation      :225-235  version 3 (:267-296): three table entries (the signed float32 component of each 10-bit code), the
//                           largest component from a float64 sum, a correctly rounded float64 sqrt and one conversion to float32;
//                           legacy (:253-262): three table entries, a float32 sum and a correctly rounded float32 sqrt
//   sh            :238-250  (b - 128) / 128: exact, so computed; [N, dim, RGB] in the file -> f_rest grouped by channel
//   the rows      :178-179, :251  every row written once, whole, in define_dtype's order; nx ny nz zero
//
// A workgroup owns SPZR_TILE consecutive rows.  It stages the tile's span of each section in LDS with 16-byte loads from the
// 16-byte boundary at or below the span (a section starts at any byte), one lane decodes one row into an LDS image whose rows
// lie row_bytes + 1 apart (a multiple of 4: every float32 is an aligned word, the three colour bytes share the last word with
// one spare byte), and the tile's contiguous output span -- rows of 71, 107, 167 or 251 bytes, so a tile starts at any byte --
// leaves in 16-byte stores gathered from that image (store_rows).  The library is built with -ffp-contract=off; every product
// and sum is spelled out anyway.
#include <cmath>

#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int SPZR_TILE = 128;   // rows per tile = threads per workgroup
constexpr int SPZR_BASE = 17;    // x y z nx ny nz f_dc_0..2 | f_rest | opacity scale_0..2 rot_0..3, then red green blue as bytes

__host__ __device__ constexpr int spzr_dim(int degree) { return degree == 1 ? 3 : (degree == 2 ? 8 : (degree == 3 ? 15 : 0)); }
__host__ __device__ constexpr int spzr_pos_bytes(int version) { return version == 1 ? 6 : 9; }
__host__ __device__ constexpr int spzr_rot_bytes(int version) { return version >= 3 ? 4 : 3; }
// a staged section: the tile's bytes behind up to 15 bytes of lead, whole quads, one spare quad (lds_u32 reads a word ahead)
__host__ __device__ constexpr int spzr_sec_quads(int per_row) { return per_row ? (SPZR_TILE * per_row + 15 + 15) / 16 + 1 : 0; }

struct SpzReadArgs {
    int64_t n;
    int64_t off[6];   // byte offsets of positions, alpha, colour, scale, rotation, sh inside the body
    float divisor;    // float32(1 << fractional_bits): inf from 128 bits on
};

// bytes [g0, g1) of `out` (16-byte aligned) <- the packed rows of RB bytes that lie RB + 1 bytes apart in the LDS image `img`
// (byte g0 is byte 0 of the image's first row), by the whole workgroup: 16-byte stores, the ragged ends byte by byte.  A word
// that runs over a row's end takes its last bytes one image byte further on.  Reads up to 8 bytes behind the last row.
template <int RB>
__device__ __forceinline__ unsigned packed_u32(const unsigned *img, int s)
{
    const int r = s / RB, c = s - r * RB;
    unsigned a = lds_u32(img, s + r);
    if (c > RB - 4) {
        const unsigned keep = (1u << (8 * (RB - c))) - 1u;
        a = (a & keep) | (lds_u32(img, s + r + 1) & ~keep);
    }
    return a;
}

template <int RB>
__device__ __forceinline__ void store_rows(unsigned char *__restrict__ out, int64_t g0, int64_t g1, const unsigned *img)
{
    const int64_t h = min(g1, (g0 + 15) & ~(int64_t)15);
    const int64_t tl = max(h, g1 & ~(int64_t)15);
    const int nh = (int)(h - g0), nt = (int)(g1 - tl), nb = (int)((tl - h) >> 4);
    const int t = threadIdx.x;
    if (t < nh) out[g0 + t] = (unsigned char)lds_u8(img, t + t / RB);
    if (t < nt) {
        const int s = (int)(tl - g0) + t;
        out[tl + t] = (unsigned char)lds_u8(img, s + s / RB);
    }
    for (int k = t; k < nb; k += blockDim.x) {
        const int s = nh + 16 * k;
        uint4 v;
        v.x = packed_u32<RB>(img, s);
        v.y = packed_u32<RB>(img, s + 4);
        v.z = packed_u32<RB>(img, s + 8);
        v.w = packed_u32<RB>(img, s + 12);
        *reinterpret_cast<uint4 *>(out + h + 16 * k) = v;
    }
}

// the sign-extended 24-bit integer / float32(1 << fractional_bits) (:193-196)
__device__ __forceinline__ unsigned spzr_fixed(unsigned u24, float divisor)
{
    const int i = (int)(u24 << 8) >> 8;
    return __float_as_uint(__fdiv_rn((float)i, divisor));
}

template <int V, int DEG>
__global__ __launch_bounds__(SPZR_TILE) void spz_unpack_kernel(const uint4 *__restrict__ body, SpzReadArgs A, const unsigned *__restrict__ tab,
                                                               unsigned char *__restrict__ out)
{
    constexpr int DIM = spzr_dim(DEG), NC = 3 * DIM, RW = SPZR_BASE + NC + 1, RB = 4 * RW - 1;
    constexpr int PB = spzr_pos_bytes(V), QB = spzr_rot_bytes(V);
    constexpr int Q_POS = 0, Q_ALPHA = Q_POS + spzr_sec_quads(PB), Q_COL = Q_ALPHA + spzr_sec_quads(1), Q_SCALE = Q_COL + spzr_sec_quads(3);
    constexpr int Q_ROT = Q_SCALE + spzr_sec_quads(3), Q_SH = Q_ROT + spzr_sec_quads(QB), Q_IMG = Q_SH + spzr_sec_quads(3 * DIM);
    extern __shared__ uint4 sr_lds[];
    const int64_t t0 = (int64_t)blockIdx.x * SPZR_TILE;
    if (t0 >= A.n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)SPZR_TILE, A.n - t0);
    const int b_pos = spz_stage_tile(body, PB, t0, cnt, sr_lds + Q_POS, A.off[0]);
    const int b_alpha = spz_stage_tile(body, 1, t0, cnt, sr_lds + Q_ALPHA, A.off[1]);
    const int b_col = spz_stage_tile(body, 3, t0, cnt, sr_lds + Q_COL, A.off[2]);
    const int b_scale = spz_stage_tile(body, 3, t0, cnt, sr_lds + Q_SCALE, A.off[3]);
    const int b_rot = spz_stage_tile(body, QB, t0, cnt, sr_lds + Q_ROT, A.off[4]);
    const int b_sh = DIM ? spz_stage_tile(body, 3 * DIM, t0, cnt, sr_lds + Q_SH, A.off[5]) : 0;
    unsigned *img = reinterpret_cast<unsigned *>(sr_lds + Q_IMG);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < cnt) {
        unsigned *o = img + r * RW;
        constexpr int tail = 9 + NC;   // o[tail] = opacity, then scale_0..2, rot_0..3, the colour bytes
        const unsigned *pos = reinterpret_cast<const unsigned *>(sr_lds + Q_POS);
        const int qp = b_pos + PB * r;
        if (V == 1) {
            const unsigned w0 = lds_u32(pos, qp), w1 = lds_u32(pos, qp + 4);
            o[0] = half_bits(w0 & 0xffffu);
            o[1] = half_bits(w0 >> 16);
            o[2] = half_bits(w1 & 0xffffu);
        } else {
            const unsigned w0 = lds_u32(pos, qp), w1 = lds_u32(pos, qp + 4), w2 = lds_u8(pos, qp + 8);
            o[0] = spzr_fixed(w0 & 0xffffffu, A.divisor);
            o[1] = spzr_fixed((w0 >> 24) | ((w1 & 0xffffu) << 8), A.divisor);
            o[2] = spzr_fixed((w1 >> 16) | (w2 << 16), A.divisor);
        }
        o[3] = o[4] = o[5] = 0u;                                                  // normals: np.zeros
        const unsigned col = lds_u32(reinterpret_cast<const unsigned *>(sr_lds + Q_COL), b_col + 3 * r);
        unsigned rgb = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned b = (col >> (8 * a)) & 0xffu;
            o[6 + a] = tab[GSX_SPZ_TAB_DC + b];
            rgb |= tab[GSX_SPZ_TAB_RGB + b] << (8 * a);
        }
        o[tail + 8] = rgb;
        o[tail] = tab[GSX_SPZ_TAB_OPA + lds_u8(reinterpret_cast<const unsigned *>(sr_lds + Q_ALPHA), b_alpha + r)];
        const unsigned sc = lds_u32(reinterpret_cast<const unsigned *>(sr_lds + Q_SCALE), b_scale + 3 * r);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            o[tail + 1 + a] = __float_as_uint(__fsub_rn(__fmul_rn((float)((sc >> (8 * a)) & 0xffu), 0.0625f), 10.0f));
        const unsigned rot = lds_u32(reinterpret_cast<const unsigned *>(sr_lds + Q_ROT), b_rot + QB * r);
        if (V >= 3) {
            const unsigned f0 = tab[GSX_SPZ_TAB_ROT3 + ((rot >> 20) & 0x3ffu)], f1 = tab[GSX_SPZ_TAB_ROT3 + ((rot >> 10) & 0x3ffu)];
            const unsigned f2 = tab[GSX_SPZ_TAB_ROT3 + (rot & 0x3ffu)];
            const double v0 = (double)__uint_as_float(f0), v1 = (double)__uint_as_float(f1), v2 = (double)__uint_as_float(f2);
            const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(v0, v0), __dmul_rn(v1, v1)), __dmul_rn(v2, v2));
            const unsigned m = __float_as_uint(__double2float_rn(__dsqrt_rn(fmax(0.0, __dsub_rn(1.0, s2)))));
            const unsigned idx = rot >> 30;                                        // 0..3 = X Y Z W holds the largest component
            const unsigned x = idx == 0 ? m : f0;
            const unsigned y = idx == 0 ? f0 : (idx == 1 ? m : f1);
            const unsigned z = idx <= 1 ? f1 : (idx == 2 ? m : f2);
            const unsigned w = idx == 3 ? m : f2;
            o[tail + 4] = w, o[tail + 5] = x, o[tail + 6] = y, o[tail + 7] = z;
        } else {
            const unsigned fx = tab[GSX_SPZ_TAB_ROTL + (rot & 0xffu)], fy = tab[GSX_SPZ_TAB_ROTL + ((rot >> 8) & 0xffu)];
            const unsigned fz = tab[GSX_SPZ_TAB_ROTL + ((rot >> 16) & 0xffu)];
            const float x = __uint_as_float(fx), y = __uint_as_float(fy), z = __uint_as_float(fz);
            const float s2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
            o[tail + 4] = __float_as_uint(__builtin_sqrtf(fmaxf(0.0f, __fsub_rn(1.0f, s2))));   // correctly rounded (see sog_math.h)
            o[tail + 5] = fx, o[tail + 6] = fy, o[tail + 7] = fz;
        }
        if (DIM) {
            const unsigned *sh = reinterpret_cast<const unsigned *>(sr_lds + Q_SH);
            const int qs = b_sh + 3 * DIM * r;
#pragma unroll
            for (int k4 = 0; k4 < (3 * DIM + 3) / 4; ++k4) {
                const unsigned w = lds_u32(sh, qs + 4 * k4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = 4 * k4 + i;                                      // byte k = coefficient k / 3 of channel k % 3
                    if (k < 3 * DIM)
                        o[9 + (k % 3) * DIM + k / 3] = __float_as_uint(__fmul_rn((float)((int)((w >> (8 * i)) & 0xffu) - 128), 0.0078125f));
                }
            }
        }
    }
    __syncthreads();
    const int64_t g0 = t0 * RB;
    store_rows<RB>(out, g0, g0 + (int64_t)cnt * RB, img);
}

template <int V, int DEG>
static void spzr_launch(gsx_ctx *c, const void *body, const SpzReadArgs &A, const void *tab, void *out)
{
    const unsigned tiles = (unsigned)((A.n + SPZR_TILE - 1) / SPZR_TILE);
    const int dim = spzr_dim(DEG), rw = SPZR_BASE + 3 * dim + 1;
    const int quads = spzr_sec_quads(spzr_pos_bytes(V)) + spzr_sec_quads(1) + 2 * spzr_sec_quads(3) + spzr_sec_quads(spzr_rot_bytes(V))
                      + spzr_sec_quads(3 * dim);
    const size_t lds = (size_t)quads * 16 + ((size_t)SPZR_TILE * rw * 4 + 15) / 16 * 16 + 16;
    hipLaunchKernelGGL((spz_unpack_kernel<V, DEG>), dim3(tiles), dim3(SPZR_TILE), lds, c->stream, static_cast<const uint4 *>(body), A,
                       static_cast<const unsigned *>(tab), static_cast<unsigned char *>(out));
}

template <int V>
static void spzr_launch_degree(gsx_ctx *c, int degree, const void *body, const SpzReadArgs &A, const void *tab, void *out)
{
    if (degree == 0) spzr_launch<V, 0>(c, body, A, tab, out);
    else if (degree == 1) spzr_launch<V, 1>(c, body, A, tab, out);
    else if (degree == 2) spzr_launch<V, 2>(c, body, A, tab, out);
    else spzr_launch<V, 3>(c, body, A, tab, out);
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_spz_unpack_dev(gsx_ctx *c, const void *body_dev, int64_t body_bytes, int version, int sh_degree, int fractional_bits,
                       const void *tables_dev, void *out_dev, int64_t n)
{
    if (!c) GSX_FAIL("gsx_spz_unpack_dev: null argument");
    if (version < 1 || version > 3 || sh_degree < 0 || sh_degree > 3 || fractional_bits < 0 || fractional_bits > 255)
        GSX_FAIL("gsx_spz_unpack_dev: version %d, SH degree %d, %d fractional bits (1 ... 3, 0 ... 3, 0 ... 255 are supported)", version,
                 sh_degree, fractional_bits);
    if (n < 0 || n >= (1LL << 32) || body_bytes < 0) GSX_FAIL("gsx_spz_unpack_dev: bad row count or body size");
    if (n == 0) return 0;
    if (!body_dev || !tables_dev || !out_dev) GSX_FAIL("gsx_spz_unpack_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(body_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(tables_dev) & 3))
        GSX_FAIL("gsx_spz_unpack_dev: body and output must be 16-byte aligned, the tables 4-byte aligned");
    const int per_row[6] = {spzr_pos_bytes(version), 1, 3, 3, spzr_rot_bytes(version), 3 * spzr_dim(sh_degree)};
    SpzReadArgs A;
    A.n = n;
    int64_t off = 0;
    for (int s = 0; s < 6; ++s) {
        A.off[s] = off;
        off += n * per_row[s];
    }
    if (off > body_bytes)
        GSX_FAIL("gsx_spz_unpack_dev: %lld rows of version %d, degree %d need %lld body bytes, %lld are there", (long long)n, version,
                 sh_degree, (long long)off, (long long)body_bytes);
    A.divisor = fractional_bits < 128 ? std::ldexp(1.0f, fractional_bits) : INFINITY;
    GSX_HIP(hipSetDevice(c->device));
    if (version == 1) spzr_launch_degree<1>(c, sh_degree, body_dev, A, tables_dev, out_dev);
    else if (version == 2) spzr_launch_degree<2>(c, sh_degree, body_dev, A, tables_dev, out_dev);
    else spzr_launch_degree<3>(c, sh_degree, body_dev, A, tables_dev, out_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
