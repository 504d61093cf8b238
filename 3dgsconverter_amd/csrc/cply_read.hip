// cply_read.hip -- the compressed-PLY reader's decode: chunk, vertex and sh rows as they lie in the file -> the reference's
// float32 rows, bit for bit.
//
// Replaces, in gsconverter/formats/compressed_ply.py (CompressedPlyFormat.read):
//   per-chunk loop          :63-122   one workgroup per tile of a 256-splat chunk, the chunk's 18 bounds broadcast through LDS
//   positions, scales       :75-103   (nv / t) * f32(max - min) + min in float64, rounded once   -> cply_denorm
//                           :342-351
//   colour                  :106-116  (n / 255.0) * f32(max - min) + min, then (cr - 0.5) / SH_C0 -> cply_dc
//                           :353-362
//   opacity                 :118-120  log(clip(na / 255, 1e-6, 1 - 1e-6) / (1 - that))           -> a 256-entry table
//   rotation                :84-89    _unpack_quaternions (:364-378)                               -> cply_quat
//                           :364-378
//   sh                      :122-127  (u8 / 256.0 - 0.5) * 8.0                                     -> a 256-entry table
//
// The arithmetic is numpy's: `max - min` is a float32 subtraction of two np.float32 scalars, everything after it float64 with
// one final rounding to float32 (the library is built with -ffp-contract=off; the operations are spelled out anyway).  Every
// quotient that takes few values comes from a table the host builds with numpy (nv / 2047, nv / 1023, n / 255.0, the
// quaternion's (v / 1023 - 0.5) / SQRT2_2, the opacity logit, the sh bytes), so the device divides only in the colour's
// `/ SH_C0` and takes one float64 square root per row, both correctly rounded.
//
// NaN bits: x86 returns the first NaN operand, quieted, and an invalid operation (inf - inf, inf * 0) gives the negative
// default NaN; the casts f32 <-> f64 keep the payload.  Traced through the statements above that is: a NaN max gives max's
// bits, quieted; else a NaN min gives min's; any other NaN is 0xffc00000.  The device's own NaN bits differ, so a NaN result
// is replaced on a cold path (x86_nan).
//
// A tile's output rows are staged in LDS and leave in 16-byte stores; its sh rows (45 bytes at degree 3, any alignment) come
// in through LDS too (row_tile.h).  Rows past 256 x chunks are not decoded (the reference's loop never reaches them).
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int CPLY_READ_CHUNK = 256;   // :12 CHUNK_SIZE
constexpr int CPLY_READ_BOUNDS = 18;   // min_x .. max_b
constexpr int CPLY_READ_BASE = 17;     // x y z nx ny nz f_dc_0..2 opacity scale_0..2 rot_0..3
constexpr int CPLY_READ_MAX_SH = GSX_CPLY_READ_MAX_SH;
constexpr int CPLY_READ_LDS = 65536;   // LDS budget of a tile: staged sh rows + output rows
constexpr double CPLY_SH_C0 = 0.28209479177387814;

struct CplyReadArgs {
    int64_t chunk_stride, vertex_stride;
    int sh_stride, n_sh, row_words, tile_rows, tiles_per_chunk, sh_lds_quads;
    int chunk_off[CPLY_READ_BOUNDS];
    int vertex_off[4];
    int sh_off[CPLY_READ_MAX_SH];
};

struct CplyReadTables {
    const double *q2047, *q1023, *q255, *dq;
    const float *opa, *sh;
};

// :346-347 `(nv / t) * (v_max - v_min) + v_min` with q = nv / t, in float64
__device__ __forceinline__ double cply_denorm(double q, float mn, float mx)
{
    const float d = __fsub_rn(mx, mn);
    return __dadd_rn(__dmul_rn(q, (double)d), (double)mn);
}

__device__ __forceinline__ float cply_f32(double r, float mn, float mx)
{
    const float o = __double2float_rn(r);
    return o == o ? o : __uint_as_float(x86_nan(mx, mn));
}

// :108-110 `(cr - 0.5) / SH_C0` on the float64 colour
__device__ __forceinline__ float cply_dc(double q, float mn, float mx)
{
    const double cr = cply_denorm(q, mn, mx);
    return cply_f32(__ddiv_rn(__dsub_rn(cr, 0.5), CPLY_SH_C0), mn, mx);
}

// :364-378: the four components of a packed rotation word
__device__ __forceinline__ void cply_quat(unsigned w, const double *__restrict__ dq, float q[4])
{
    const int largest = (int)(w >> 30);
    const double dv0 = dq[(w >> 20) & 0x3ffu], dv1 = dq[(w >> 10) & 0x3ffu], dv2 = dq[w & 0x3ffu];
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(dv0, dv0), __dmul_rn(dv1, dv1)), __dmul_rn(dv2, dv2));
    const double m = __dsqrt_rn(fmin(fmax(__dsub_rn(1.0, s), 0.0), 1.0));   // np.sqrt(np.clip(1.0 - (...), 0, 1))
    const float fm = __double2float_rn(m), f0 = __double2float_rn(dv0), f1 = __double2float_rn(dv1), f2 = __double2float_rn(dv2);
    q[0] = largest == 0 ? fm : f0;
    q[1] = largest == 0 ? f0 : (largest == 1 ? fm : f1);
    q[2] = largest <= 1 ? f1 : (largest == 2 ? fm : f2);
    q[3] = largest == 3 ? fm : f2;
}

// one workgroup per tile of `tile_rows` rows inside one chunk; rows [0, n) are decoded
__global__ __launch_bounds__(256) void cply_unpack_kernel(const unsigned char *__restrict__ chunks, const unsigned char *__restrict__ verts,
                                                          const uint4 *__restrict__ sh, int64_t n, CplyReadArgs A, CplyReadTables T,
                                                          uint4 *__restrict__ out)
{
    extern __shared__ uint4 cr_lds[];
    __shared__ float bnd[CPLY_READ_BOUNDS];
    const int64_t tile = blockIdx.x;
    const int64_t chunk = tile / A.tiles_per_chunk;
    const int64_t r0 = chunk * CPLY_READ_CHUNK + (tile % A.tiles_per_chunk) * A.tile_rows;
    if (r0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)A.tile_rows, n - r0);
    if ((int)threadIdx.x < CPLY_READ_BOUNDS)
        bnd[threadIdx.x] = __uint_as_float(ld_u32(chunks, chunk * A.chunk_stride + A.chunk_off[threadIdx.x]));
    int sh_base = 0;
    if (A.n_sh > 0) sh_base = spz_stage_tile(sh, A.sh_stride, r0, cnt, cr_lds);
    const unsigned *sh32 = reinterpret_cast<const unsigned *>(cr_lds);
    unsigned *o32 = reinterpret_cast<unsigned *>(cr_lds + A.sh_lds_quads);
    __syncthreads();
    for (int r = threadIdx.x; r < cnt; r += blockDim.x) {
        const int64_t vb = (r0 + r) * A.vertex_stride;
        const unsigned pp = ld_u32(verts, vb + A.vertex_off[0]);
        const unsigned pr = ld_u32(verts, vb + A.vertex_off[1]);
        const unsigned ps = ld_u32(verts, vb + A.vertex_off[2]);
        const unsigned pc = ld_u32(verts, vb + A.vertex_off[3]);
        unsigned *o = o32 + r * A.row_words;
        // :75-80 positions (11 / 10 / 11 bits)
        o[0] = __float_as_uint(cply_f32(cply_denorm(T.q2047[(pp >> 21) & 0x7ffu], bnd[0], bnd[3]), bnd[0], bnd[3]));
        o[1] = __float_as_uint(cply_f32(cply_denorm(T.q1023[(pp >> 11) & 0x3ffu], bnd[1], bnd[4]), bnd[1], bnd[4]));
        o[2] = __float_as_uint(cply_f32(cply_denorm(T.q2047[pp & 0x7ffu], bnd[2], bnd[5]), bnd[2], bnd[5]));
        o[3] = o[4] = o[5] = 0u;                                                          // normals: np.zeros
        // :106-116 colour -> f_dc, alpha -> logit
        o[6] = __float_as_uint(cply_dc(T.q255[pc >> 24], bnd[12], bnd[15]));
        o[7] = __float_as_uint(cply_dc(T.q255[(pc >> 16) & 0xffu], bnd[13], bnd[16]));
        o[8] = __float_as_uint(cply_dc(T.q255[(pc >> 8) & 0xffu], bnd[14], bnd[17]));
        o[9] = __float_as_uint(T.opa[pc & 0xffu]);
        // :92-103 scales
        o[10] = __float_as_uint(cply_f32(cply_denorm(T.q2047[(ps >> 21) & 0x7ffu], bnd[6], bnd[9]), bnd[6], bnd[9]));
        o[11] = __float_as_uint(cply_f32(cply_denorm(T.q1023[(ps >> 11) & 0x3ffu], bnd[7], bnd[10]), bnd[7], bnd[10]));
        o[12] = __float_as_uint(cply_f32(cply_denorm(T.q2047[ps & 0x7ffu], bnd[8], bnd[11]), bnd[8], bnd[11]));
        // :84-89 rotation
        float q[4];
        cply_quat(pr, T.dq, q);
#pragma unroll
        for (int a = 0; a < 4; ++a) o[13 + a] = __float_as_uint(q[a]);
        // :122-127 sh
        const int sq = sh_base + r * A.sh_stride;
        for (int k = 0; k < A.n_sh; ++k) o[CPLY_READ_BASE + k] = __float_as_uint(T.sh[lds_u8(sh32, sq + A.sh_off[k])]);
    }
    __syncthreads();
    // the tile's rows are contiguous in the output and start on a 16-byte boundary (tile_rows is a multiple of 4)
    const int words = cnt * A.row_words, quads = words >> 2;
    uint4 *dst = out + (r0 * A.row_words >> 2);
    const uint4 *src = reinterpret_cast<const uint4 *>(o32);
    for (int k = threadIdx.x; k < quads; k += blockDim.x) dst[k] = src[k];
    if ((int)threadIdx.x < (words & 3)) reinterpret_cast<unsigned *>(dst + quads)[threadIdx.x] = o32[4 * quads + threadIdx.x];
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_cply_unpack_dev(gsx_ctx *c, const void *chunk_dev, int64_t n_chunks, const void *vertex_dev, int64_t n_vertices, const void *sh_dev,
                        const gsx_cply_read_layout *layout, const void *tables_dev, float *out_dev)
{
    if (!c || !layout) GSX_FAIL("gsx_cply_unpack_dev: null argument");
    if (n_chunks < 0 || n_vertices < 0 || n_vertices >= (1LL << 40)) GSX_FAIL("gsx_cply_unpack_dev: bad row counts");
    const int64_t n = std::min(n_vertices, n_chunks * CPLY_READ_CHUNK);
    const gsx_cply_read_layout &l = *layout;
    if (l.n_sh < 0 || l.n_sh > CPLY_READ_MAX_SH) GSX_FAIL("gsx_cply_unpack_dev: %d sh properties (0 ... %d are supported)", l.n_sh, CPLY_READ_MAX_SH);
    if (n > 0 && (!chunk_dev || !vertex_dev || !tables_dev || !out_dev || (l.n_sh > 0 && !sh_dev))) GSX_FAIL("gsx_cply_unpack_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(sh_dev) & 15) || (reinterpret_cast<uintptr_t>(tables_dev) & 7))
        GSX_FAIL("gsx_cply_unpack_dev: output and sh rows must be 16-byte aligned, tables 8-byte aligned");
    CplyReadArgs A;
    A.chunk_stride = l.chunk_stride;
    A.vertex_stride = l.vertex_stride;
    A.sh_stride = (int)l.sh_stride;
    A.n_sh = l.n_sh;
    A.row_words = CPLY_READ_BASE + l.n_sh;
    if (l.chunk_stride < 4 * CPLY_READ_BOUNDS || l.vertex_stride < 16 || (l.n_sh > 0 && (l.sh_stride < l.n_sh || l.sh_stride > 4096)))
        GSX_FAIL("gsx_cply_unpack_dev: row strides chunk %lld, vertex %lld, sh %lld", (long long)l.chunk_stride, (long long)l.vertex_stride,
                 (long long)l.sh_stride);
    for (int f = 0; f < CPLY_READ_BOUNDS; ++f) {
        if (l.chunk_offset[f] < 0 || l.chunk_offset[f] + 4 > l.chunk_stride) GSX_FAIL("gsx_cply_unpack_dev: chunk field %d at offset %d", f, l.chunk_offset[f]);
        A.chunk_off[f] = l.chunk_offset[f];
    }
    for (int f = 0; f < 4; ++f) {
        if (l.vertex_offset[f] < 0 || l.vertex_offset[f] + 4 > l.vertex_stride) GSX_FAIL("gsx_cply_unpack_dev: vertex field %d at offset %d", f, l.vertex_offset[f]);
        A.vertex_off[f] = l.vertex_offset[f];
    }
    for (int k = 0; k < CPLY_READ_MAX_SH; ++k) {
        if (k < l.n_sh && (l.sh_offset[k] < 0 || l.sh_offset[k] >= l.sh_stride)) GSX_FAIL("gsx_cply_unpack_dev: sh field %d at offset %d", k, l.sh_offset[k]);
        A.sh_off[k] = k < l.n_sh ? l.sh_offset[k] : 0;
    }
    // rows per tile: a power of two (so it divides the chunk), at least 4 (16-byte aligned tiles), staged sh + output <= 64 KiB
    int tr = CPLY_READ_CHUNK;
    auto lds_bytes = [&](int t) { return (l.n_sh > 0 ? spz_in_bytes(t, A.sh_stride) : 0) + (size_t)t * A.row_words * 4; };
    while (tr > 4 && lds_bytes(tr) > (size_t)CPLY_READ_LDS) tr >>= 1;
    if (lds_bytes(tr) > (size_t)CPLY_READ_LDS) GSX_FAIL("gsx_cply_unpack_dev: rows too wide for a tile");
    A.tile_rows = tr;
    A.tiles_per_chunk = CPLY_READ_CHUNK / tr;
    A.sh_lds_quads = l.n_sh > 0 ? (int)(spz_in_bytes(tr, A.sh_stride) / 16) : 0;
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    const double *td = static_cast<const double *>(tables_dev);
    CplyReadTables T;
    T.q2047 = td + GSX_CPLY_TAB_Q2047;
    T.q1023 = td + GSX_CPLY_TAB_Q1023;
    T.q255 = td + GSX_CPLY_TAB_Q255;
    T.dq = td + GSX_CPLY_TAB_DQ;
    T.opa = reinterpret_cast<const float *>(td + GSX_CPLY_TAB_DOUBLES) + GSX_CPLY_TAB_OPA;
    T.sh = reinterpret_cast<const float *>(td + GSX_CPLY_TAB_DOUBLES) + GSX_CPLY_TAB_SH;
    const int64_t chunks_used = (n + CPLY_READ_CHUNK - 1) / CPLY_READ_CHUNK;
    const int64_t tiles = (chunks_used - 1) * A.tiles_per_chunk + (n - (chunks_used - 1) * CPLY_READ_CHUNK + tr - 1) / tr;
    if (tiles >= (1LL << 31)) GSX_FAIL("gsx_cply_unpack_dev: too many rows");
    hipLaunchKernelGGL(cply_unpack_kernel, dim3((unsigned)tiles), dim3(std::max(64, std::min(256, tr))), lds_bytes(tr), c->stream,
                       static_cast<const unsigned char *>(chunk_dev), static_cast<const unsigned char *>(vertex_dev), static_cast<const uint4 *>(sh_dev),
                       n, A, T, reinterpret_cast<uint4 *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
