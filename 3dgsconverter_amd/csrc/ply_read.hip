// ply_read.hip -- the 3DGS / CloudCompare PLY readers' row transcode: the vertex element's rows as they lie in a binary file ->
// the reference's packed rows, bit for bit.
//
// Replaces, in gsconverter/formats/ply_3dgs.py (Ply3DGSFormat.read) and gsconverter/formats/ply_cc.py (PlyCCFormat.read):
//   the zeroed table        ply_3dgs.py:45    ply_cc.py:45     a field without a source writes zero
//   the mapping loop        ply_3dgs.py:48-58 ply_cc.py:48-60  `converted_data[target] = vertices[source]`, up to 65 strided column
//                                                              copies -> one pass over the rows, driven by a descriptor table
// Which source a target takes (prefix detection, extra fields, the third lookup of the CloudCompare reader) is the host's
// business (formats/ply_reader.py: plan); the two readers share this kernel.
//
// numpy's `dst[field] = src[field]` converts by value.  A float32 target takes
//   f4             the bits, moved as an integer (a signalling NaN or a denormal stays as it is)
//   f8             x86's conversion: round to nearest even, overflow to +-inf, subnormal results kept, a NaN keeps its sign and
//                  the top 22 payload bits and is quieted -- v_cvt_f32_f64 does all of that (ply_f64_to_f32)
//   i1 u1 i2 u2    exact
//   i4 u4          round to nearest even (v_cvt_f32_i32 / v_cvt_f32_u32 under the default rounding mode)
// red green blue and the extra fields are byte copies (GSX_PLY_T_RAW; the host refuses a source of another type).  A
// big-endian body is byte-swapped field by field as it is read.
//
// A workgroup of 256 lanes owns a tile of consecutive rows (spz_tile_rows on the larger stride: 128 rows, or 64 when a stride is
// over 256 bytes; four waves a tile, because two tiles of up to 32 KiB in LDS leave room for two workgroups a CU): the tile's raw
// bytes are staged in LDS with
// 16-byte loads from any starting byte, consecutive lanes take consecutive fields of a row -- consecutive LDS words on the
// canonical layouts -- and write into an LDS image of the output tile, which leaves in 16-byte stores (row_tile.h).  The
// descriptors are one word per field in the kernel argument struct.
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int PLYR_MAX_FIELDS = GSX_PLY_READ_MAX_FIELDS;

struct PlyReadArgs {
    int in_stride, out_stride, n_fields, big_endian, in_quads, tile_rows;
    unsigned desc[PLYR_MAX_FIELDS];           // src offset (10 bits, PLY_NO_SRC = none) | type << 10 | dst offset << 14 | dst bytes << 24
};

__host__ __device__ inline unsigned ply_swap32(unsigned w) { return (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24); }

// (ply_f64_to_f32, the float64 -> float32 cast, lives in row_tile.h: the Parquet reader casts with it too)

// the output bytes of one field, as up to two little-endian words: W(q) is the little-endian u32 at byte q of the staged rows
template <class W>
__host__ __device__ inline void ply_field(const W &word, int q, unsigned type, unsigned nb, bool be, unsigned &w0, unsigned &w1)
{
    w1 = 0u;
    switch (type) {
    case GSX_PLY_T_RAW:
        w0 = word(q);
        if (nb == 8) w1 = word(q + 4);
        break;
    case GSX_PLY_T_F4:
        w0 = word(q);
        if (be) w0 = ply_swap32(w0);
        break;
    case GSX_PLY_T_F8: {
        const unsigned a = word(q), b = word(q + 4);
        w0 = be ? ply_f64_to_f32(ply_swap32(b), ply_swap32(a)) : ply_f64_to_f32(a, b);
        break;
    }
    case GSX_PLY_T_I4: {
        const unsigned v = be ? ply_swap32(word(q)) : word(q);
        const float f = (float)(int)v;
        w0 = __builtin_bit_cast(unsigned, f);
        break;
    }
    case GSX_PLY_T_U4: {
        const unsigned v = be ? ply_swap32(word(q)) : word(q);
        const float f = (float)v;
        w0 = __builtin_bit_cast(unsigned, f);
        break;
    }
    case GSX_PLY_T_I2:
    case GSX_PLY_T_U2: {
        unsigned v = word(q) & 0xffffu;
        if (be) v = (v >> 8) | ((v & 0xffu) << 8);
        const float f = type == GSX_PLY_T_I2 ? (float)(int)(short)v : (float)v;
        w0 = __builtin_bit_cast(unsigned, f);
        break;
    }
    default: {   // GSX_PLY_T_I1, GSX_PLY_T_U1
        const unsigned v = word(q) & 0xffu;
        const float f = type == GSX_PLY_T_I1 ? (float)(int)(signed char)v : (float)v;
        w0 = __builtin_bit_cast(unsigned, f);
        break;
    }
    }
}

struct PlyLdsWord {
    const unsigned *lds;
    __device__ __forceinline__ unsigned operator()(int q) const { return lds_u32(lds, q); }
};

// one workgroup of PLY_THREADS lanes per tile of A.tile_rows rows; rows [0, n), row 0 at byte `first` of `body`
__global__ __launch_bounds__(PLY_THREADS) void ply_unpack_kernel(const uint4 *__restrict__ body, int64_t first, int64_t n, PlyReadArgs A,
                                                         unsigned char *__restrict__ out)
{
    extern __shared__ uint4 pr_lds[];
    const int tr = A.tile_rows;
    const int64_t t0 = (int64_t)blockIdx.x * tr;
    if (t0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)tr, n - t0);
    const int base = spz_stage_tile(body, A.in_stride, t0, cnt, pr_lds, first);
    const PlyLdsWord word{reinterpret_cast<const unsigned *>(pr_lds)};
    unsigned char *img = reinterpret_cast<unsigned char *>(pr_lds + A.in_quads);
    __syncthreads();
    const unsigned nf = (unsigned)A.n_fields;
    const unsigned pairs = (unsigned)cnt * nf;
    const bool be = A.big_endian != 0;
    for (unsigned p = threadIdx.x; p < pairs; p += PLY_THREADS) {
        const unsigned r = p / nf, f = p - r * nf;
        const unsigned d = A.desc[f];
        const unsigned so = d & 0x3ffu, type = (d >> 10) & 15u, nb = d >> 24;
        const unsigned o = r * (unsigned)A.out_stride + ((d >> 14) & 0x3ffu);
        unsigned w0 = 0u, w1 = 0u;
        if (so != (unsigned)PLY_NO_SRC) ply_field(word, base + (int)(r * (unsigned)A.in_stride + so), type, nb, be, w0, w1);
        if (nb == 4 && (o & 3u) == 0u) {
            *reinterpret_cast<unsigned *>(img + o) = w0;
        } else {
            for (unsigned i = 0; i < nb; ++i) img[o + i] = (unsigned char)((i < 4 ? w0 : w1) >> (8 * (i & 3u)));
        }
    }
    __syncthreads();
    const int64_t g0 = t0 * A.out_stride;
    store_bytes(out, g0, g0 + (int64_t)cnt * A.out_stride, img);
}

static int ply_type_bytes(int type) { return type <= GSX_PLY_T_U1 ? 1 : type <= GSX_PLY_T_U2 ? 2 : type <= GSX_PLY_T_F4 ? 4 : 8; }

// gsx_ply_read_layout -> PlyReadArgs: strides and counts in range, every source inside an input row, the output fields tile the
// output row (every byte written exactly once: nothing of the LDS image leaves unwritten)
static int ply_layout_to_args(const gsx_ply_read_layout *l, PlyReadArgs *A, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    GSX_CHECK(ply_strides(l->in_stride, l->out_stride, who));
    if (l->n_fields < 1 || l->n_fields > PLYR_MAX_FIELDS) GSX_FAIL("%s: %d fields (1 ... %d are supported)", who, l->n_fields, PLYR_MAX_FIELDS);
    if (l->big_endian != 0 && l->big_endian != 1) GSX_FAIL("%s: big_endian %d", who, l->big_endian);
    unsigned char covered[SPZ_MAX_ROW_BYTES] = {0};
    for (int f = 0; f < l->n_fields; ++f) {
        const int so = l->src_offset[f], type = l->src_type[f], dof = l->dst_offset[f], nb = l->dst_bytes[f];
        if (nb != 1 && nb != 2 && nb != 4 && nb != 8) GSX_FAIL("%s: field %d of %d bytes", who, f, nb);
        if (dof < 0 || dof + nb > l->out_stride) GSX_FAIL("%s: field %d at byte offset %d of a %d-byte output row", who, f, dof, l->out_stride);
        if (type < GSX_PLY_T_I1 || type > GSX_PLY_T_RAW) GSX_FAIL("%s: field %d has type code %d", who, f, type);
        if (type != GSX_PLY_T_RAW && nb != 4) GSX_FAIL("%s: field %d converts to float32 into %d bytes", who, f, nb);
        if (type == GSX_PLY_T_RAW && nb > 1 && l->big_endian && so >= 0) GSX_FAIL("%s: field %d is a byte copy of %d bytes from a big-endian body", who, f, nb);
        const int sb = type == GSX_PLY_T_RAW ? nb : ply_type_bytes(type);
        if (so < -1 || (so >= 0 && so + sb > l->in_stride)) GSX_FAIL("%s: field %d reads %d bytes at offset %d of a %d-byte row", who, f, sb, so, l->in_stride);
        GSX_CHECK(ply_cover(covered, dof, nb, "field", f, who));
        A->desc[f] = (unsigned)(so < 0 ? PLY_NO_SRC : so) | ((unsigned)type << 10) | ((unsigned)dof << 14) | ((unsigned)nb << 24);
    }
    A->n_fields = l->n_fields;
    A->big_endian = l->big_endian;
    return ply_args_finish(covered, "field", A->desc, l->n_fields, l->in_stride, l->out_stride, A, who);
}

struct PlyHostWord {
    const unsigned char *rows;
    unsigned operator()(int q) const { return (unsigned)rows[q] | ((unsigned)rows[q + 1] << 8) | ((unsigned)rows[q + 2] << 16) | ((unsigned)rows[q + 3] << 24); }
};

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_ply_unpack_dev(gsx_ctx *c, const void *body_dev, int64_t first_byte, int64_t n, const gsx_ply_read_layout *layout, void *out_dev)
{
    if (!c) GSX_FAIL("gsx_ply_unpack_dev: null argument");
    PlyReadArgs A;
    GSX_CHECK(ply_layout_to_args(layout, &A, "gsx_ply_unpack_dev"));
    if (n < 0 || first_byte < 0 || first_byte > 15) GSX_FAIL("gsx_ply_unpack_dev: n >= 0 and 0 <= first_byte <= 15");
    if (n == 0) return 0;
    return ply_launch(c, reinterpret_cast<const void *>(ply_unpack_kernel), A, n, body_dev, "body", out_dev, "gsx_ply_unpack_dev",
                      [&](unsigned tiles, size_t lds) {
                          hipLaunchKernelGGL(ply_unpack_kernel, dim3(tiles), dim3(PLY_THREADS), lds, c->stream, static_cast<const uint4 *>(body_dev),
                                             first_byte, n, A, static_cast<unsigned char *>(out_dev));
                      });
}

int gsx_ply_unpack_host(const void *body, int64_t n, const gsx_ply_read_layout *layout, void *out)
{
    PlyReadArgs A;
    GSX_CHECK(ply_layout_to_args(layout, &A, "gsx_ply_unpack_host"));
    if (n < 0 || (n > 0 && (!body || !out))) GSX_FAIL("gsx_ply_unpack_host: bad arguments");
    const PlyHostWord word{static_cast<const unsigned char *>(body)};
    unsigned char *o = static_cast<unsigned char *>(out);
    for (int64_t r = 0; r < n; ++r) {
        for (int f = 0; f < A.n_fields; ++f) {
            const unsigned d = A.desc[f];
            const unsigned so = d & 0x3ffu, nb = d >> 24;
            unsigned w0 = 0u, w1 = 0u;
            // (rows are walked one at a time from their own base: q stays below 2^31 for any n)
            if (so != (unsigned)PLY_NO_SRC) {
                const PlyHostWord row{word.rows + r * A.in_stride};
                ply_field(row, (int)so, (d >> 10) & 15u, nb, A.big_endian != 0, w0, w1);
            }
            unsigned char *dst = o + r * A.out_stride + ((d >> 14) & 0x3ffu);
            for (unsigned i = 0; i < nb; ++i) dst[i] = (unsigned char)((i < 4 ? w0 : w1) >> (8 * (i & 3u)));
        }
    }
    return 0;
}

}  // extern "C"
