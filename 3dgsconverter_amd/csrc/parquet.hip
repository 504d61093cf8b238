// parquet.hip -- the Parquet reader's and writer's transposes: Arrow columns -> the reference's packed rows with numpy's casts and
// the validity bitmaps applied, and a structured table's rows -> one contiguous column per field with the Arrow validity bitmap
// that `pa.Table.from_pandas` would build.  pyarrow keeps the pages, snappy, the dictionaries and Thrift.
//
// Replaces, in gsconverter/formats/parquet.py (ParquetFormat):
//   the column loop   :51-55    `converted_data[name] = df_renamed[name].values`, 62 strided column copies with a cast each (and,
//                               ahead of it, pandas' own null -> NaN pass over every column that has nulls) -> one pass, driven by
//                               a descriptor per output field                                              (parquet_rows_kernel)
//   the frame         :94-108   `pd.DataFrame(data)` + rename + reorder + `from_pandas`: a strided copy per field into a column
//                               of its own, and a NaN scan per float column for the validity bitmap and the null count -> one
//                               pass over the rows                                                      (parquet_columns_kernel)
// Which column feeds which field, the names and their order are the host's business (formats/parquet_reader.py: plan,
// formats/parquet_writer.py: plan_write).
//
// numpy's `dst[field] = column` converts by value.  A float32 target takes
//   f4               the bits, moved as an integer        f2               exact, a NaN keeps sign and payload (half_bits)
//   f8               x86's conversion (ply_f64_to_f32)    i1 u1 i2 u2      exact
//   i4 u4 i8 u8      round to nearest even, once
// a u1 target (red green blue) is a byte copy.  A row whose validity bit is cleared takes 0x7fc00000 whatever its value slot
// holds: to_pandas hands the reference np.nan there, in the column's own type, and its float32 is the positive default NaN --
// but for a float16 column, where to_pandas writes the half 0x7fff, which numpy's cast makes 0x7fffe000 (pq_null_bits).
//
// Both kernels: a workgroup of 256 lanes owns a tile of consecutive rows (spz_tile_rows: 128 rows, or 64 when the row is over 256
// bytes), the row image of the tile lies in LDS and meets global memory in 16-byte accesses (row_tile.h: spz_stage_tile on the
// way in, store_bytes on the way out).  The column side is walked a wave per (field, 64 rows): the field is wave-uniform, so its
// descriptor comes out of the kernel arguments as scalar loads, consecutive lanes take consecutive rows of one column -- one
// coalesced 64 / 128 / 256 / 512-byte access -- and a wave's 64 rows are exactly one word of an Arrow bitmap: the reader loads
// its validity as one uniform 8-byte word, the writer's ballot IS the word, stored whole by one lane.  No atomics touch a bitmap.
//
// LDS banking.  Lane <-> row walks the image at the row stride: 248 bytes = 62 dwords.  ds_write_b32 and ds_read_b32 bank a
// 32-lane half at (a / 4) mod 32, and 62 l = 30 l (mod 32) puts lanes l and l + 16 on one bank: a 2-way conflict, on every
// dword of the canonical table (251-byte rows with rgb move as bytes and dwords by turns and fare no better).  One dword of
// padding a row -- a stride of 63 dwords, odd, so 32 lanes fall on 32 banks -- would remove it (two dwords would make it 64,
// the worst stride there is).  But a padded image is no longer the tile's bytes as they lie in the table: store_bytes /
// spz_stage_tile could not move it as one span, and the 16-byte side -- the one that meets HBM -- would need a re-gather of
// its own through LDS.  The image stays UNPADDED.  What that costs is an ESTIMATE, no counter was read: a 128-row tile of 62
// fields is 124 wave-wide LDS accesses of two halves each, 2 cycles instead of 1 per half = ~250 extra LDS cycles a tile,
// against the ~32 KiB of HBM traffic each way that the same tile costs (several thousand cycles at a CU's share of the
// bandwidth), with other resident workgroups to hide behind.  Measured is only that the kernels are 0.02-0.6 % of their calls,
// which the host link and pyarrow's codec bound (profiles/parquet_10m.txt).
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int PQ_MAX_FIELDS = GSX_PARQUET_MAX_FIELDS;
constexpr int PQ_THREADS = 256;

__host__ __device__ inline int pq_type_bytes(int type)
{
    switch (type) {
    case GSX_PLY_T_I1: case GSX_PLY_T_U1: return 1;
    case GSX_PLY_T_I2: case GSX_PLY_T_U2: case GSX_PARQUET_T_F2: return 2;
    case GSX_PLY_T_I4: case GSX_PLY_T_U4: case GSX_PLY_T_F4: return 4;
    default: return 8;   // GSX_PLY_T_F8, GSX_PARQUET_T_I8, GSX_PARQUET_T_U8
    }
}

// the float32 bits of one source value (lo, hi: its little-endian words, the unused high bytes of a narrow value ignored)
__host__ __device__ inline unsigned pq_cast(unsigned type, unsigned lo, unsigned hi)
{
    float f;
    switch (type) {
    case GSX_PLY_T_F4: return lo;
    case GSX_PLY_T_F8: return ply_f64_to_f32(lo, hi);
    case GSX_PARQUET_T_F2: return half_bits(lo & 0xffffu);
    case GSX_PLY_T_I1: f = (float)(int)(signed char)(lo & 0xffu); break;
    case GSX_PLY_T_U1: f = (float)(lo & 0xffu); break;
    case GSX_PLY_T_I2: f = (float)(int)(short)(lo & 0xffffu); break;
    case GSX_PLY_T_U2: f = (float)(lo & 0xffffu); break;
    case GSX_PLY_T_I4: f = (float)(int)lo; break;
    case GSX_PLY_T_U4: f = (float)lo; break;
    case GSX_PARQUET_T_I8: f = (float)(long long)(((unsigned long long)hi << 32) | lo); break;
    default: f = (float)(((unsigned long long)hi << 32) | lo); break;   // GSX_PARQUET_T_U8
    }
    return __builtin_bit_cast(unsigned, f);
}

// what a null reads as
__host__ __device__ inline unsigned pq_null_bits(unsigned type) { return type == GSX_PARQUET_T_F2 ? 0x7fffe000u : 0x7fc00000u; }

// is this value a NaN (kind 1: float32 in lo, kind 2: float64 in lo, hi)?
__host__ __device__ inline bool pq_is_nan(int kind, unsigned lo, unsigned hi)
{
    if (kind == 1) return (lo & 0x7fffffffu) > 0x7f800000u;
    const unsigned h = hi & 0x7fffffffu;
    return h > 0x7ff00000u || (h == 0x7ff00000u && lo != 0u);
}

struct PqRowsArgs {
    int out_stride, n_fields, tile_rows;
    unsigned desc[PQ_MAX_FIELDS];             // type (4 bits; bit 4: no source) | dst offset << 5 | dst bytes << 15
    int64_t col[PQ_MAX_FIELDS];               // byte offset of the column's values in the column buffer
    int64_t valid[PQ_MAX_FIELDS];             // byte offset of its bitmap, -1 = every row is valid
};

struct PqColsArgs {
    int in_stride, n_fields, tile_rows;
    unsigned desc[PQ_MAX_FIELDS];             // src offset (10 bits) | bytes << 10 | kind << 14
    int64_t col[PQ_MAX_FIELDS];               // byte offset of the column in the output buffer
    int64_t valid[PQ_MAX_FIELDS];             // byte offset of its bitmap there, -1 = none
};

// columns -> rows.  One workgroup per tile of A.tile_rows rows (a multiple of 64); rows [0, n)
__global__ __launch_bounds__(PQ_THREADS) void parquet_rows_kernel(const unsigned char *__restrict__ cols, int64_t n, PqRowsArgs A,
                                                                  unsigned char *__restrict__ out)
{
    extern __shared__ uint4 pq_lds[];
    unsigned char *img = reinterpret_cast<unsigned char *>(pq_lds);
    const int tr = A.tile_rows;
    const int64_t t0 = (int64_t)blockIdx.x * tr;
    if (t0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)tr, n - t0);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int words = tr >> 6, items = A.n_fields * words;
    for (int it = wave; it < items; it += PQ_THREADS / 64) {
        const int f = it / words, h = it - f * words;
        const unsigned d = A.desc[f];
        const unsigned type = d & 15u, nb = d >> 15;
        const bool no_src = (d >> 4) & 1u;
        const int r = h * 64 + lane;
        if (h * 64 >= cnt) continue;   // (uniform)
        unsigned long long vbits = ~0ull;
        if (!no_src && A.valid[f] >= 0) vbits = *reinterpret_cast<const unsigned long long *>(cols + A.valid[f] + 8 * ((t0 >> 6) + h));
        if (r >= cnt) continue;
        const int64_t row = t0 + r;
        unsigned w0 = 0u, w1 = 0u;
        if (!no_src) {
            const unsigned char *src = cols + A.col[f];
            if (nb != 4) {                                   // a byte copy of 1, 2 or 8 bytes (GSX_PLY_T_RAW)
                if (nb == 1) w0 = src[row];
                else if (nb == 2) w0 = reinterpret_cast<const unsigned short *>(src)[row];
                else { const uint2 v = reinterpret_cast<const uint2 *>(src)[row]; w0 = v.x; w1 = v.y; }
            } else if (type == GSX_PLY_T_RAW) {
                w0 = reinterpret_cast<const unsigned *>(src)[row];
            } else {
                unsigned lo, hi = 0u;
                switch (pq_type_bytes((int)type)) {
                case 1: lo = src[row]; break;
                case 2: lo = reinterpret_cast<const unsigned short *>(src)[row]; break;
                case 4: lo = reinterpret_cast<const unsigned *>(src)[row]; break;
                default: { const uint2 v = reinterpret_cast<const uint2 *>(src)[row]; lo = v.x; hi = v.y; break; }
                }
                w0 = ((vbits >> lane) & 1ull) ? pq_cast(type, lo, hi) : pq_null_bits(type);
            }
        }
        const unsigned o = (unsigned)r * (unsigned)A.out_stride + ((d >> 5) & 0x3ffu);
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

// rows -> columns.  One workgroup per tile of A.tile_rows rows (a multiple of 64); rows [0, n)
__global__ __launch_bounds__(PQ_THREADS) void parquet_columns_kernel(const uint4 *__restrict__ rows, int64_t n, PqColsArgs A,
                                                                     unsigned char *__restrict__ out, unsigned long long *__restrict__ nulls)
{
    extern __shared__ uint4 pq_lds[];
    const int tr = A.tile_rows;
    const int64_t t0 = (int64_t)blockIdx.x * tr;
    if (t0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)tr, n - t0);
    const int base = spz_stage_tile(rows, A.in_stride, t0, cnt, pq_lds);
    const unsigned *lds = reinterpret_cast<const unsigned *>(pq_lds);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int words = tr >> 6, items = A.n_fields * words;
    for (int it = wave; it < items; it += PQ_THREADS / 64) {
        const int f = it / words, h = it - f * words;
        if (h * 64 >= cnt) continue;   // (uniform: no row of the table in these 64, and no bitmap word for them either)
        const unsigned d = A.desc[f];
        const int so = (int)(d & 0x3ffu), nb = (int)((d >> 10) & 15u), kind = (int)(d >> 14);
        const int r = h * 64 + lane;
        const bool active = r < cnt;
        unsigned w0 = 0u, w1 = 0u;
        if (active) {
            const int q = base + r * A.in_stride + so;
            w0 = lds_u32(lds, q);
            if (nb == 8) w1 = lds_u32(lds, q + 4);
            unsigned char *dst = out + A.col[f];
            const int64_t row = t0 + r;
            if (nb == 4) reinterpret_cast<unsigned *>(dst)[row] = w0;
            else if (nb == 8) reinterpret_cast<uint2 *>(dst)[row] = make_uint2(w0, w1);
            else if (nb == 2) reinterpret_cast<unsigned short *>(dst)[row] = (unsigned short)w0;
            else dst[row] = (unsigned char)w0;
        }
        if (kind) {                                          // (uniform)
            const bool nan = active && pq_is_nan(kind, w0, w1);
            const unsigned long long vword = __ballot(active && !nan);   // bit l = row t0 + 64 h + l is valid; past n: zero
            const unsigned long long nword = __ballot(nan);
            if (lane == 0) {
                *reinterpret_cast<unsigned long long *>(out + A.valid[f] + 8 * ((t0 >> 6) + h)) = vword;
                if (nword) atomicAdd(nulls + f, (unsigned long long)__popcll(nword));
            }
        }
    }
}

static int pq_tile(gsx_ctx *c, int64_t n, int stride, int *tr, unsigned *tiles, const char *who)
{
    *tr = spz_tile_rows(stride);
    const int64_t t = (n + *tr - 1) / *tr;
    if (t >= (1LL << 31)) GSX_FAIL("%s: too many rows", who);
    *tiles = (unsigned)t;
    return 0;
}

static int pq_rows_args(const gsx_parquet_rows_layout *l, int64_t n, int64_t cols_bytes, PqRowsArgs *A, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (l->out_stride < 1 || l->out_stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("%s: rows of %d bytes (1 ... %d are supported)", who, l->out_stride, SPZ_MAX_ROW_BYTES);
    if (l->n_fields < 1 || l->n_fields > PQ_MAX_FIELDS) GSX_FAIL("%s: %d fields (1 ... %d are supported)", who, l->n_fields, PQ_MAX_FIELDS);
    unsigned char covered[SPZ_MAX_ROW_BYTES] = {0};
    const int64_t bitmap_bytes = (n + 63) / 64 * 8;
    for (int f = 0; f < l->n_fields; ++f) {
        const int type = l->src_type[f], dof = l->dst_offset[f], nb = l->dst_bytes[f];
        const int64_t co = l->col_offset[f], vo = l->valid_offset[f];
        if (nb != 1 && nb != 2 && nb != 4 && nb != 8) GSX_FAIL("%s: field %d of %d bytes", who, f, nb);
        if (dof < 0 || dof + nb > l->out_stride) GSX_FAIL("%s: field %d at byte offset %d of a %d-byte output row", who, f, dof, l->out_stride);
        if (type < GSX_PLY_T_I1 || type > GSX_PARQUET_T_F2) GSX_FAIL("%s: field %d has type code %d", who, f, type);
        if (type != GSX_PLY_T_RAW && nb != 4) GSX_FAIL("%s: field %d converts to float32 into %d bytes", who, f, nb);
        GSX_CHECK(ply_cover(covered, dof, nb, "field", f, who));
        if (co < 0) {
            if (co != -1) GSX_FAIL("%s: field %d has column offset %lld", who, f, (long long)co);
        } else {
            const int sb = type == GSX_PLY_T_RAW ? nb : pq_type_bytes(type);
            if ((co & 15) || co + n * sb > cols_bytes) GSX_FAIL("%s: field %d reads %lld values of %d bytes at byte %lld of %lld (16-byte aligned)", who, f, (long long)n, sb, (long long)co, (long long)cols_bytes);
            if (vo < -1 || (vo >= 0 && ((vo & 7) || vo + bitmap_bytes > cols_bytes || type == GSX_PLY_T_RAW)))
                GSX_FAIL("%s: field %d has its bitmap of %lld bytes at byte %lld of %lld (8-byte aligned, converted fields only)", who, f, (long long)bitmap_bytes, (long long)vo, (long long)cols_bytes);
        }
        A->desc[f] = (unsigned)type | (co < 0 ? 16u : 0u) | ((unsigned)dof << 5) | ((unsigned)nb << 15);
        A->col[f] = co < 0 ? 0 : co;
        A->valid[f] = co < 0 ? -1 : vo;
    }
    for (int i = 0; i < l->out_stride; ++i)
        if (!covered[i]) GSX_FAIL("%s: output byte %d belongs to no field", who, i);
    for (int f = l->n_fields; f < PQ_MAX_FIELDS; ++f) { A->desc[f] = 0u; A->col[f] = 0; A->valid[f] = -1; }
    A->out_stride = l->out_stride;
    A->n_fields = l->n_fields;
    A->tile_rows = 0;
    return 0;
}

static int pq_cols_args(const gsx_parquet_columns_layout *l, int64_t n, int64_t out_bytes, PqColsArgs *A, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (l->in_stride < 1 || l->in_stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("%s: rows of %d bytes (1 ... %d are supported)", who, l->in_stride, SPZ_MAX_ROW_BYTES);
    if (l->n_fields < 1 || l->n_fields > PQ_MAX_FIELDS) GSX_FAIL("%s: %d fields (1 ... %d are supported)", who, l->n_fields, PQ_MAX_FIELDS);
    const int64_t bitmap_bytes = (n + 63) / 64 * 8;
    for (int f = 0; f < l->n_fields; ++f) {
        const int so = l->src_offset[f], nb = l->bytes[f], kind = l->kind[f];
        const int64_t co = l->col_offset[f], vo = l->valid_offset[f];
        if (nb != 1 && nb != 2 && nb != 4 && nb != 8) GSX_FAIL("%s: field %d of %d bytes", who, f, nb);
        if (so < 0 || so + nb > l->in_stride) GSX_FAIL("%s: field %d reads %d bytes at offset %d of a %d-byte row", who, f, nb, so, l->in_stride);
        if (kind < 0 || kind > 2 || (kind == 1 && nb != 4) || (kind == 2 && nb != 8)) GSX_FAIL("%s: field %d of %d bytes has kind %d", who, f, nb, kind);
        if (co < 0 || (co & 15) || co + n * nb > out_bytes) GSX_FAIL("%s: column %d of %lld values of %d bytes at byte %lld of %lld (16-byte aligned)", who, f, (long long)n, nb, (long long)co, (long long)out_bytes);
        if (kind && (vo < 0 || (vo & 7) || vo + bitmap_bytes > out_bytes)) GSX_FAIL("%s: bitmap %d of %lld bytes at byte %lld of %lld (8-byte aligned)", who, f, (long long)bitmap_bytes, (long long)vo, (long long)out_bytes);
        A->desc[f] = (unsigned)so | ((unsigned)nb << 10) | ((unsigned)kind << 14);
        A->col[f] = co;
        A->valid[f] = kind ? vo : -1;
    }
    for (int f = l->n_fields; f < PQ_MAX_FIELDS; ++f) { A->desc[f] = 0u; A->col[f] = 0; A->valid[f] = -1; }
    A->in_stride = l->in_stride;
    A->n_fields = l->n_fields;
    A->tile_rows = 0;
    return 0;
}

static unsigned pq_host_word(const unsigned char *p, int nb)
{
    unsigned w = 0u;
    for (int i = 0; i < nb && i < 4; ++i) w |= (unsigned)p[i] << (8 * i);
    return w;
}

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_parquet_rows_dev(gsx_ctx *c, const void *cols_dev, int64_t cols_bytes, int64_t n, const gsx_parquet_rows_layout *layout, void *out_dev)
{
    if (!c) GSX_FAIL("gsx_parquet_rows_dev: null argument");
    if (n < 0 || cols_bytes < 0) GSX_FAIL("gsx_parquet_rows_dev: n >= 0 and cols_bytes >= 0");
    PqRowsArgs A;
    GSX_CHECK(pq_rows_args(layout, n, cols_bytes, &A, "gsx_parquet_rows_dev"));
    if (n == 0) return 0;
    if (!cols_dev || !out_dev) GSX_FAIL("gsx_parquet_rows_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(cols_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        GSX_FAIL("gsx_parquet_rows_dev: columns and output must be 16-byte aligned");
    unsigned tiles;
    GSX_CHECK(pq_tile(c, n, A.out_stride, &A.tile_rows, &tiles, "gsx_parquet_rows_dev"));
    const size_t lds = ((size_t)A.tile_rows * A.out_stride + 32 + 15) / 16 * 16;   // + what store_bytes reads behind the image
    GSX_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(parquet_rows_kernel, dim3(tiles), dim3(PQ_THREADS), lds, c->stream, static_cast<const unsigned char *>(cols_dev), n, A,
                       static_cast<unsigned char *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_parquet_rows_host(const void *cols, int64_t cols_bytes, int64_t n, const gsx_parquet_rows_layout *layout, void *out)
{
    if (n < 0 || cols_bytes < 0) GSX_FAIL("gsx_parquet_rows_host: n >= 0 and cols_bytes >= 0");
    PqRowsArgs A;
    GSX_CHECK(pq_rows_args(layout, n, cols_bytes, &A, "gsx_parquet_rows_host"));
    if (n > 0 && (!cols || !out)) GSX_FAIL("gsx_parquet_rows_host: null argument");
    const unsigned char *cb = static_cast<const unsigned char *>(cols);
    unsigned char *o = static_cast<unsigned char *>(out);
    for (int64_t r = 0; r < n; ++r) {
        for (int f = 0; f < A.n_fields; ++f) {
            const unsigned d = A.desc[f];
            const unsigned type = d & 15u, nb = d >> 15;
            unsigned w0 = 0u, w1 = 0u;
            if (!((d >> 4) & 1u)) {
                const int sb = type == GSX_PLY_T_RAW ? (int)nb : pq_type_bytes((int)type);
                const unsigned char *p = cb + A.col[f] + r * sb;
                const unsigned lo = pq_host_word(p, sb), hi = sb == 8 ? pq_host_word(p + 4, 4) : 0u;
                if (type == GSX_PLY_T_RAW) {
                    w0 = lo;
                    w1 = hi;
                } else {
                    const bool valid = A.valid[f] < 0 || ((cb[A.valid[f] + (r >> 3)] >> (r & 7)) & 1u);
                    w0 = valid ? pq_cast(type, lo, hi) : pq_null_bits(type);
                }
            }
            unsigned char *dst = o + r * A.out_stride + ((d >> 5) & 0x3ffu);
            for (unsigned i = 0; i < nb; ++i) dst[i] = (unsigned char)((i < 4 ? w0 : w1) >> (8 * (i & 3u)));
        }
    }
    return 0;
}

int gsx_parquet_columns_dev(gsx_ctx *c, const void *rows_dev, int64_t n, const gsx_parquet_columns_layout *layout, void *out_dev, int64_t out_bytes,
                            uint64_t *null_counts_dev)
{
    if (!c) GSX_FAIL("gsx_parquet_columns_dev: null argument");
    if (n < 0 || out_bytes < 0) GSX_FAIL("gsx_parquet_columns_dev: n >= 0 and out_bytes >= 0");
    PqColsArgs A;
    GSX_CHECK(pq_cols_args(layout, n, out_bytes, &A, "gsx_parquet_columns_dev"));
    if (!null_counts_dev) GSX_FAIL("gsx_parquet_columns_dev: null argument");
    GSX_HIP(hipSetDevice(c->device));
    GSX_HIP(hipMemsetAsync(null_counts_dev, 0, sizeof(uint64_t) * PQ_MAX_FIELDS, c->stream));
    if (n == 0) return 0;
    if (!rows_dev || !out_dev) GSX_FAIL("gsx_parquet_columns_dev: null argument");
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(null_counts_dev) & 7))
        GSX_FAIL("gsx_parquet_columns_dev: rows and output must be 16-byte aligned");
    unsigned tiles;
    GSX_CHECK(pq_tile(c, n, A.in_stride, &A.tile_rows, &tiles, "gsx_parquet_columns_dev"));
    const size_t lds = spz_in_bytes(A.tile_rows, A.in_stride);
    hipLaunchKernelGGL(parquet_columns_kernel, dim3(tiles), dim3(PQ_THREADS), lds, c->stream, static_cast<const uint4 *>(rows_dev), n, A,
                       static_cast<unsigned char *>(out_dev), reinterpret_cast<unsigned long long *>(null_counts_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_parquet_columns_host(const void *rows, int64_t n, const gsx_parquet_columns_layout *layout, void *out, int64_t out_bytes, uint64_t *null_counts)
{
    if (n < 0 || out_bytes < 0) GSX_FAIL("gsx_parquet_columns_host: n >= 0 and out_bytes >= 0");
    PqColsArgs A;
    GSX_CHECK(pq_cols_args(layout, n, out_bytes, &A, "gsx_parquet_columns_host"));
    if (!null_counts || (n > 0 && (!rows || !out))) GSX_FAIL("gsx_parquet_columns_host: null argument");
    for (int f = 0; f < PQ_MAX_FIELDS; ++f) null_counts[f] = 0;
    const unsigned char *rb = static_cast<const unsigned char *>(rows);
    unsigned char *o = static_cast<unsigned char *>(out);
    const int64_t bitmap_bytes = (n + 63) / 64 * 8;
    for (int f = 0; f < A.n_fields; ++f) {
        const unsigned d = A.desc[f];
        const int so = (int)(d & 0x3ffu), nb = (int)((d >> 10) & 15u), kind = (int)(d >> 14);
        if (kind) memset(o + A.valid[f], 0, (size_t)bitmap_bytes);
        for (int64_t r = 0; r < n; ++r) {
            const unsigned char *p = rb + r * A.in_stride + so;
            memcpy(o + A.col[f] + r * nb, p, (size_t)nb);
            if (kind) {
                if (pq_is_nan(kind, pq_host_word(p, 4), nb == 8 ? pq_host_word(p + 4, 4) : 0u)) ++null_counts[f];
                else o[A.valid[f] + (r >> 3)] |= (unsigned char)(1u << (r & 7));
            }
        }
    }
    return 0;
}

}  // extern "C"
