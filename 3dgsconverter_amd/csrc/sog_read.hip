// sog_read.hip -- the SOG reader's decode: the decoded RGBA texels of a .sog bundle -> the reference's rows
// (GaussianStruct.define_dtype(has_scal=False, has_rgb=False)), bit for bit.
//
// Replaces, in gsconverter/formats/sog.py (SogFormat.read):
//   positions     :67-86    the u16 code of each axis from the low and the high texel -> a float32 table of 65 536 entries per axis
//                           that the host builds with numpy (float64 there, rounded once on assignment: no device exp)
//   scales        :92-102   a codebook look-up per channel
//   rotation      :106-142  three table entries ((b / 255 - 0.5) * 2, float32, the host's), a float32 sum of squares taken left
//                           to right, 1 - sum, max(., 0), a correctly rounded float32 sqrt; the slot is uint8(alpha - 252): an
//                           alpha byte below 252 matches no slot and the four components stay 0
//   f_dc, opacity :147-158  a codebook look-up per channel; a 256-entry opacity table (numpy's own log, the host's)
//   shN           :183-225  label = r | g << 8; f_rest_{ch C + j} = codebook[channel ch of centroid pixel (label, j)].  The pixel is
//                           the READER's: (label / 64) * (64 * 3 C) + (label % 64) * C + j; the host uploads only the first 64 C
//                           pixels of every image row, so here it is pixel label * C + j
//   the rows      :234-245  every row written once, whole, in define_dtype's order; nx ny nz zero
//
// A workgroup walks tiles of SOGR_TILE consecutive rows.  The five 256-entry tables sit in LDS for the workgroup's life.  Per
// tile one lane decodes one row's texels (one aligned 32-bit load per texture, coalesced) into an LDS image of packed rows and
// leaves the row's label in LDS; then consecutive lanes take consecutive coefficients j of one row, so that a row's C
// consecutive centroid pixels arrive as one request; the tile's contiguous output span leaves through store_bytes in 16-byte
// stores.  A label >= the palette's size sets *flag and reads nothing.  The library is built with -ffp-contract=off; every
// product and sum is spelled out anyway.
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int SOGR_TILE = 128;      // rows per tile
constexpr int SOGR_THREADS = 256;   // threads per workgroup
constexpr int SOGR_BASE = 17;       // x y z nx ny nz f_dc_0..2 | f_rest | opacity scale_0..2 rot_0..3
constexpr int SOGR_TAB_WORDS = 5 * 256;

__host__ __device__ constexpr int sogr_coeffs(int bands) { return bands == 1 ? 3 : (bands == 2 ? 8 : (bands == 3 ? 15 : 0)); }
// LDS: the tables | the tile's labels | the image of packed rows + 32 spare bytes (store_bytes reads up to 19 bytes behind it)
__host__ __device__ constexpr size_t sogr_lds_bytes(int bands)
{
    return 4 * (size_t)(SOGR_TAB_WORDS + SOGR_TILE + SOGR_TILE * (SOGR_BASE + 3 * sogr_coeffs(bands))) + 32;
}

struct SogReadArgs {
    int64_t n;
    const unsigned *tex[7];   // means_l means_u scales quats sh0 shN_labels (n texels each) | the compacted centroid pixels
    const unsigned *tab;      // GSX_SOG_TAB_*: 1280 words, then the position table [3][65536]
    unsigned palette;         // labels must be below it
    unsigned *flag;
};

template <int BANDS>
__global__ __launch_bounds__(SOGR_THREADS) void sog_unpack_kernel(SogReadArgs A, unsigned char *__restrict__ out)
{
    constexpr int C = sogr_coeffs(BANDS), NC = 3 * C, RW = SOGR_BASE + NC, RB = 4 * RW;
    extern __shared__ uint4 so_lds[];
    unsigned *tab = reinterpret_cast<unsigned *>(so_lds);
    unsigned *lab = tab + SOGR_TAB_WORDS;
    unsigned *img = lab + SOGR_TILE;
    const int t = threadIdx.x;
    for (int k = t; k < SOGR_TAB_WORDS; k += SOGR_THREADS) tab[k] = A.tab[k];
    const unsigned *__restrict__ pos = A.tab + GSX_SOG_TAB_POS;
    const int64_t tiles = (A.n + SOGR_TILE - 1) / SOGR_TILE;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();   // the tables are there; the tile before has left the image
        const int64_t t0 = tile * SOGR_TILE;
        const int cnt = (int)min((int64_t)SOGR_TILE, A.n - t0);
        if (t < cnt) {
            const int64_t row = t0 + t;
            unsigned *o = img + t * RW;
            constexpr int tail = 9 + NC;   // o[tail] = opacity, then scale_0..2, rot_0..3
            const unsigned lo = A.tex[0][row], hi = A.tex[1][row];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                o[a] = pos[a * 65536 + (((lo >> (8 * a)) & 0xffu) | (((hi >> (8 * a)) & 0xffu) << 8))];
            o[3] = o[4] = o[5] = 0u;                                                // normals: np.zeros
            const unsigned sc = A.tex[2][row], dc = A.tex[4][row];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                o[tail + 1 + a] = tab[GSX_SOG_TAB_SCALE + ((sc >> (8 * a)) & 0xffu)];
                o[6 + a] = tab[GSX_SOG_TAB_SH0 + ((dc >> (8 * a)) & 0xffu)];
            }
            o[tail] = tab[GSX_SOG_TAB_OPA + (dc >> 24)];
            const unsigned q = A.tex[3][row];
            const unsigned u0 = tab[GSX_SOG_TAB_QUAT + (q & 0xffu)], u1 = tab[GSX_SOG_TAB_QUAT + ((q >> 8) & 0xffu)];
            const unsigned u2 = tab[GSX_SOG_TAB_QUAT + ((q >> 16) & 0xffu)];
            const float c0 = __uint_as_float(u0), c1 = __uint_as_float(u1), c2 = __uint_as_float(u2);
            const float s2 = __fadd_rn(__fadd_rn(__fmul_rn(c0, c0), __fmul_rn(c1, c1)), __fmul_rn(c2, c2));
            const unsigned cm = __float_as_uint(__builtin_sqrtf(fmaxf(__fsub_rn(1.0f, s2), 0.0f)));   // correctly rounded (see sog_math.h)
            const unsigned mc = ((q >> 24) - 252u) & 0xffu;                         // uint8 arithmetic: below 252 wraps to 4 ... 255
            const bool slot = mc < 4u;
            o[tail + 4] = !slot ? 0u : (mc == 0 ? cm : u0);
            o[tail + 5] = !slot ? 0u : (mc == 0 ? u0 : (mc == 1 ? cm : u1));
            o[tail + 6] = !slot ? 0u : (mc <= 1 ? u1 : (mc == 2 ? cm : u2));
            o[tail + 7] = !slot ? 0u : (mc == 3 ? cm : u2);
            if (BANDS) {
                const unsigned l = A.tex[5][row] & 0xffffu;
                lab[t] = l;
                if (l >= A.palette) *A.flag = 1u;
            }
        }
        __syncthreads();
        if (BANDS) {
            for (int k = t; k < cnt * C; k += SOGR_THREADS) {
                const int r = k / C, j = k - r * C;
                const unsigned l = lab[r];
                unsigned *o = img + r * RW + 9 + j;
                if (l < A.palette) {
                    const unsigned px = A.tex[6][(int64_t)l * C + j];
                    o[0] = tab[GSX_SOG_TAB_SHN + (px & 0xffu)];
                    o[C] = tab[GSX_SOG_TAB_SHN + ((px >> 8) & 0xffu)];
                    o[2 * C] = tab[GSX_SOG_TAB_SHN + ((px >> 16) & 0xffu)];
                } else {
                    o[0] = o[C] = o[2 * C] = 0u;                                    // (the host raises: these rows are never returned)
                }
            }
            __syncthreads();
        }
        const int64_t g0 = t0 * RB;
        store_bytes(out, g0, g0 + (int64_t)cnt * RB, reinterpret_cast<const unsigned char *>(img));
    }
}

template <int BANDS>
static void sogr_launch(gsx_ctx *c, const SogReadArgs &A, void *out)
{
    const unsigned blocks = tile_blocks(c, A.n, SOGR_TILE, 8);
    hipLaunchKernelGGL((sog_unpack_kernel<BANDS>), dim3(blocks), dim3(SOGR_THREADS), sogr_lds_bytes(BANDS), c->stream, A,
                       static_cast<unsigned char *>(out));
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_sog_unpack_dev(gsx_ctx *c, const void *texels_dev, int64_t texels_bytes, const int64_t *offsets, int bands, int64_t palette,
                       const void *tables_dev, void *out_dev, int64_t n, uint32_t *flag_dev)
{
    if (!c || !offsets) GSX_FAIL("gsx_sog_unpack_dev: null argument");
    if (bands < 0 || bands > 3) GSX_FAIL("gsx_sog_unpack_dev: %d bands (0 ... 3 are supported)", bands);
    if (bands && (palette < 1 || palette > 65536)) GSX_FAIL("gsx_sog_unpack_dev: a palette of %lld entries (1 ... 65536)", (long long)palette);
    if (n < 0 || n >= (1LL << 32) || texels_bytes < 0) GSX_FAIL("gsx_sog_unpack_dev: bad row count or texel size");
    if (n == 0) return 0;
    if (!texels_dev || !tables_dev || !out_dev || !flag_dev) GSX_FAIL("gsx_sog_unpack_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(texels_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(tables_dev) & 3)
        || (reinterpret_cast<uintptr_t>(flag_dev) & 3))
        GSX_FAIL("gsx_sog_unpack_dev: texels and output must be 16-byte aligned, the tables and the flag 4-byte aligned");
    SogReadArgs A;
    A.n = n;
    const int coeffs = sogr_coeffs(bands);
    for (int k = 0; k < 7; ++k) {
        A.tex[k] = nullptr;
        if (k >= 5 && !bands) continue;
        const int64_t need = k < 6 ? 4 * n : 4 * palette * coeffs;
        if (offsets[k] < 0 || (offsets[k] & 3) || offsets[k] > texels_bytes || need > texels_bytes - offsets[k])
            GSX_FAIL("gsx_sog_unpack_dev: texture %d at byte %lld needs %lld bytes, %lld are there", k, (long long)offsets[k], (long long)need,
                     (long long)texels_bytes);
        A.tex[k] = reinterpret_cast<const unsigned *>(static_cast<const unsigned char *>(texels_dev) + offsets[k]);
    }
    A.tab = static_cast<const unsigned *>(tables_dev);
    A.palette = bands ? (unsigned)palette : 0u;
    A.flag = flag_dev;
    GSX_HIP(hipSetDevice(c->device));
    if (bands == 0) sogr_launch<0>(c, A, out_dev);
    else if (bands == 1) sogr_launch<1>(c, A, out_dev);
    else if (bands == 2) sogr_launch<2>(c, A, out_dev);
    else sogr_launch<3>(c, A, out_dev);
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
