// splat_read.hip -- the .splat reader's decode: the file's 32-byte records -> the reference's rows
// (GaussianStruct.define_dtype(has_scal=False, has_rgb=True, sh_degree=0), packed: 17 float32 and three bytes, 71 bytes), bit
// for bit.
//
// Replaces, in gsconverter/formats/splat.py (SplatFormat.read):
//   positions   :38-40         the file's bits, moved as integers (a signalling NaN or a denormal stays as it is)
//   scales      :43-48         np.log(np.maximum(s, 1e-6)): the maximum with the NaN test written out (np.maximum hands a NaN
//                              on, fmaxf does not; negative, -0 and denormal scales become 1e-6f), numpy's own float32 log
//                              (np_log.h)
//   rotation    :52-63         (b - 128) / 128 is exact; the sum of four squares is exact in float32 in any order (integers
//                              <= 65536 over 16384); a correctly rounded sqrt, max(norm, 1e-6f) (reached only when all four
//                              bytes are 128), one IEEE division each
//   opacity     :67-69         a 256-entry float32 table the host builds with numpy (no device log of a float64 chain)
//   colour      :75-77         a 256-entry float32 table, likewise
//   the rows    :35-36         nx ny nz and red green blue stay zero: the reference never assigns them
//
// A workgroup owns SPLR_TILE consecutive records: its input starts at a multiple of 4096 bytes, its output at a multiple of
// 128 * 71 = 9088 = 568 * 16 bytes.  One lane loads one record as two 16-byte loads, decodes it and writes its packed 71-byte
// row into an LDS image (17 aligned words cut from the row's 18 with the row's byte shift, the ragged ends byte by byte), and
// the image leaves in 16-byte stores (store_bytes; only the last tile has a tail).  The library is built with
// -ffp-contract=off; every product and sum is spelled out anyway.
#include "gsx_common.h"
#include "np_log.h"
#include "row_tile.h"

namespace gsx {

constexpr int SPLR_TILE = 128;    // records per tile = threads per workgroup
constexpr int SPLR_REC = 32;      // bytes per record: 3 f32 position | 3 f32 scale | 4 u8 colour (r g b alpha) | 4 u8 rotation
constexpr int SPLR_WORDS = 18;    // x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3, then red green blue and no fourth byte
constexpr int SPLR_ROW = 4 * SPLR_WORDS - 1;
constexpr int SPLR_LDS = SPLR_TILE * SPLR_ROW + 32;   // the image + what store_bytes reads behind it (up to 19 bytes)
static_assert(SPLR_REC == 2 * sizeof(uint4) && (SPLR_TILE * SPLR_ROW) % 16 == 0 && SPLR_LDS % 16 == 0, "a record is two quads; tiles start on quads");

// np.log(np.maximum(s, 1e-6)) (:43-48)
__device__ __forceinline__ unsigned splr_scale(unsigned bits)
{
    const float s = __uint_as_float(bits);
    return __float_as_uint(np_logf(s != s ? s : (s > 1e-6f ? s : 1e-6f)));
}

// the row's 18 words (the last one holds three bytes) -> bytes [71 r, 71 r + 71) of the image: the 17 aligned words inside that
// span, then the 0 ... 3 bytes before and after them
__device__ __forceinline__ void splr_put_row(unsigned char *img, int r, const unsigned (&w)[SPLR_WORDS])
{
    const int b = SPLR_ROW * r;
    const int nh = (4 - (b & 3)) & 3;                       // bytes of w[0] before the first aligned word
    unsigned *a = reinterpret_cast<unsigned *>(img + b + nh);
#pragma unroll
    for (int k = 0; k < SPLR_WORDS - 1; ++k) a[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], (unsigned)nh);
    for (int i = 0; i < nh; ++i) img[b + i] = (unsigned char)(w[0] >> (8 * i));
    for (int i = nh + 4 * (SPLR_WORDS - 1); i < SPLR_ROW; ++i) img[b + i] = (unsigned char)(w[SPLR_WORDS - 1] >> (8 * (i & 3)));
}

__global__ __launch_bounds__(SPLR_TILE) void splat_unpack_kernel(const uint4 *__restrict__ recs, int64_t n, const unsigned *__restrict__ tab,
                                                                 unsigned char *__restrict__ out)
{
    __shared__ uint4 img4[SPLR_LDS / 16];
    unsigned char *img = reinterpret_cast<unsigned char *>(img4);
    const int64_t t0 = (int64_t)blockIdx.x * SPLR_TILE;
    if (t0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)SPLR_TILE, n - t0);
    const int r = threadIdx.x;
    if (r < cnt) {
        const uint4 lo = recs[2 * (t0 + r)], hi = recs[2 * (t0 + r) + 1];
        unsigned w[SPLR_WORDS];
        w[0] = lo.x, w[1] = lo.y, w[2] = lo.z;                                   // :38-40
        w[3] = w[4] = w[5] = 0u;                                                 // normals: np.zeros
        const unsigned col = hi.z, rot = hi.w;
#pragma unroll
        for (int a = 0; a < 3; ++a) w[6 + a] = tab[GSX_SPLAT_TAB_DC + ((col >> (8 * a)) & 0xffu)];   // :75-77
        w[9] = tab[GSX_SPLAT_TAB_OPA + (col >> 24)];                             // :67-69
        w[10] = splr_scale(lo.w), w[11] = splr_scale(hi.x), w[12] = splr_scale(hi.y);
        float q[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) q[a] = __fmul_rn((float)((int)((rot >> (8 * a)) & 0xffu) - 128), 0.0078125f);   // :52-55, exact
        float ss = __fmul_rn(q[0], q[0]);
#pragma unroll
        for (int a = 1; a < 4; ++a) ss = __fadd_rn(ss, __fmul_rn(q[a], q[a]));   // :58 (exact)
        float norm = __builtin_sqrtf(ss);   // correctly rounded (HIP's __fsqrt_rn is the native v_sqrt_f32 here, 1 ulp off at times)
        norm = norm > 1e-6f ? norm : 1e-6f;                                      // :59
#pragma unroll
        for (int a = 0; a < 4; ++a) w[13 + a] = __float_as_uint(__fdiv_rn(q[a], norm));   // :60-63
        w[17] = 0u;                                                              // red green blue: never assigned
        splr_put_row(img, r, w);
    }
    __syncthreads();
    const int64_t g0 = t0 * SPLR_ROW;
    store_bytes(out, g0, g0 + (int64_t)cnt * SPLR_ROW, img);
}

// np.log of every input, element by element (the devtool's proof and the GPU tests)
__global__ void np_log_math_kernel(const float *__restrict__ x, int64_t n, unsigned *__restrict__ out)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = __float_as_uint(np_logf(x[i]));
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_splat_unpack_dev(gsx_ctx *c, const void *recs_dev, int64_t n, const float *tables_dev, void *out_dev)
{
    if (!c) GSX_FAIL("gsx_splat_unpack_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_splat_unpack_dev: 0 <= n < 2^32");
    if (n == 0) return 0;
    if (!recs_dev || !tables_dev || !out_dev) GSX_FAIL("gsx_splat_unpack_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(recs_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(tables_dev) & 3))
        GSX_FAIL("gsx_splat_unpack_dev: records and output must be 16-byte aligned, the tables 4-byte aligned");
    GSX_HIP(hipSetDevice(c->device));
    const unsigned tiles = (unsigned)((n + SPLR_TILE - 1) / SPLR_TILE);
    hipLaunchKernelGGL(splat_unpack_kernel, dim3(tiles), dim3(SPLR_TILE), 0, c->stream, static_cast<const uint4 *>(recs_dev), n,
                       reinterpret_cast<const unsigned *>(tables_dev), static_cast<unsigned char *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_np_log_math_dev(gsx_ctx *c, const float *x_dev, int64_t n, uint32_t *out_bits_dev)
{
    if (!c || (n > 0 && (!x_dev || !out_bits_dev))) GSX_FAIL("gsx_np_log_math_dev: null argument");
    if (n < 0) GSX_FAIL("gsx_np_log_math_dev: n < 0");
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    hipLaunchKernelGGL(np_log_math_kernel, dim3(tile_blocks(c, n, 256, 16)), dim3(256), 0, c->stream, x_dev, n, out_bits_dev);
    GSX_HIP(hipGetLastError());
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gsx_np_logf_host(const float *x, float *out, int64_t n)
{
    if (n > 0 && (!x || !out)) GSX_FAIL("gsx_np_logf_host: null argument");
    for (int64_t i = 0; i < n; ++i) out[i] = np_logf(x[i]);
    return 0;
}

}  // extern "C"
