// ksplat_read.hip -- the .ksplat reader's decode: the sections' interleaved splat rows as they lie in the file -> the reference's
// float32 rows, bit for bit.
//
// Replaces, in gsconverter/formats/ksplat.py (KSplatFormat.read):
//   row -> bucket           :148-156  i / bucketSize for the rows of the full buckets, then a search in the prefix sums of the
//                                     partially filled buckets' lengths (found once per tile, refined per lane)
//   raw rows                :161-197  a tile's bytes staged in LDS with 16-byte loads (rows of 24 ... 140 bytes, any alignment)
//   position                :200-210  level 0: the bits; else (f32(u16) - f32(range)) * sf + centre, three float32 roundings
//   scale                   :213-219  level 0: the bits; else float16 -> float32 (a signalling NaN stays signalling: numpy's cast)
//   rotation                :222-226  level 0: the bits; else ((f32(u16) - 32767.5f) / 32767.5f) * 1.41421356f
//   colour, opacity         :229-234  two 256-entry float32 tables the host builds with numpy ((b / 255 - 0.5) / SH_C0, the logit)
//   sh                      :249-261  level 0: the bits; level 1: float16 -> float32; level >= 2: (f32(u8) - 128) / 128
//   consolidation           :266-315  every row written once at its place in the output table (define_dtype's field order), the
//                                     fields its section does not carry (nx ny nz, f_rest beyond its sh_count) zero
//
// Level 0 moves bits, never floats.  The library is built with -ffp-contract=off; the float32 operations are spelled out anyway.
//
// NaN bits of a position: x86 quiets the NaN operand it returns and gives the negative default NaN for an invalid operation
// (0 * inf, inf - inf); where both operands of numpy's float32 add are NaN the reference's rows carry the second one's bits
// (the golden cases with NaN block sizes and NaN centres pin this).  Traced through `(pos_u - sr) * sf + centre` (pos_u - sr is
// always finite): a NaN centre gives the centre's bits, quieted; else a NaN sf gives sf's bits, quieted; else 0 * inf and
// inf - inf give 0xffc00000.  The device's own NaN bits differ, so a NaN result is replaced on a cold path (x86_nan).
//
// One launch per section.  A tile's output rows are staged in LDS and leave in 16-byte stores; a tile need not start on a
// 16-byte boundary of the output (sections of any row count follow each other), so the words before the first and after the
// last whole quad are stored one by one.
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int KSR_TILE = 128;          // rows per tile = threads per workgroup
constexpr int KSR_BASE = 17;           // x y z nx ny nz f_dc_0..2 | f_rest | opacity scale_0..2 rot_0..3

struct KsReadArgs {
    int64_t rows_off, cen_off, n, out_row, full_rows, prefix_off;
    unsigned bucket_size, n_full, n_partial, n_buckets;
    int sh_count, row_bytes, row_words, n_coeffs, in_quads;
    float sr, sf;
};

// :209-210 `(pos_u - sr) * sf + centre`
__device__ __forceinline__ unsigned ksr_position(unsigned u16, float sr, float sf, float c)
{
    const float t2 = __fmul_rn(__fsub_rn((float)u16, sr), sf);
    const float r = __fadd_rn(t2, c);
    return r == r ? __float_as_uint(r) : x86_nan(c, sf);
}

// the first j in [lo, hi] with prefix[j] > i (hi if none: the host has checked that the lengths cover every row)
__device__ __forceinline__ int ksr_search(const unsigned *__restrict__ prefix, int lo, int hi, int64_t i)
{
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)prefix[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// LV: 0 = compression level 0, 1 = level 1, 2 = level >= 2.  One workgroup per tile of KSR_TILE rows of one section.
template <int LV>
__global__ __launch_bounds__(KSR_TILE) void ksplat_unpack_kernel(const uint4 *__restrict__ body, KsReadArgs A, const unsigned *__restrict__ prefix,
                                                                 const float *__restrict__ tab, unsigned *__restrict__ out)
{
    extern __shared__ uint4 kr_lds[];
    __shared__ int jr[2];
    const int64_t t0 = (int64_t)blockIdx.x * KSR_TILE;
    prefix += A.prefix_off;
    if (t0 >= A.n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)KSR_TILE, A.n - t0);
    const int in_base = spz_stage_tile(body, A.row_bytes, t0, cnt, kr_lds, A.rows_off);
    if (LV >= 1 && threadIdx.x < 2) {
        const int64_t i = threadIdx.x == 0 ? t0 : t0 + cnt - 1;
        jr[threadIdx.x] = (i < A.full_rows || A.n_partial == 0) ? 0 : ksr_search(prefix, 0, (int)A.n_partial - 1, i);
    }
    const unsigned *in32 = reinterpret_cast<const unsigned *>(kr_lds);
    unsigned *o32 = reinterpret_cast<unsigned *>(kr_lds + A.in_quads);
    const int64_t gw0 = (A.out_row + t0) * A.row_words;   // the tile's first output word
    const int pad = (int)(gw0 & 3);
    __syncthreads();
    const int r = threadIdx.x;
    if (r < cnt) {
        const int q = in_base + r * A.row_bytes;
        unsigned *o = o32 + pad + r * A.row_words;
        const int rest = 9, tail = 9 + A.n_coeffs;   // o[tail] = opacity, then scale_0..2, rot_0..3
        unsigned colour;
        int sh_q;
        if (LV == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                o[a] = lds_u32(in32, q + 4 * a);
                o[tail + 1 + a] = lds_u32(in32, q + 12 + 4 * a);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) o[tail + 4 + a] = lds_u32(in32, q + 24 + 4 * a);
            colour = lds_u32(in32, q + 40);
            sh_q = q + 44;
        } else {
            const int64_t i = t0 + r;
            int64_t b;
            if (i < A.full_rows) b = (unsigned)i / A.bucket_size;
            else b = (int64_t)A.n_full + (A.n_partial ? ksr_search(prefix, jr[0], jr[1], i) : 0);
            b = min(b, (int64_t)A.n_buckets - 1);
            const unsigned char *bytes = reinterpret_cast<const unsigned char *>(body);
            const unsigned w0 = lds_u32(in32, q), w1 = lds_u32(in32, q + 4), w2 = lds_u32(in32, q + 8);
            const unsigned w3 = lds_u32(in32, q + 12), w4 = lds_u32(in32, q + 16);
            const unsigned p[3] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu};
            const unsigned s[3] = {w1 >> 16, w2 & 0xffffu, w2 >> 16};
            const unsigned t[4] = {w3 & 0xffffu, w3 >> 16, w4 & 0xffffu, w4 >> 16};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float c = __uint_as_float(ld_u32(bytes, A.cen_off + 12 * b + 4 * a));
                o[a] = ksr_position(p[a], A.sr, A.sf, c);
                o[tail + 1 + a] = half_bits(s[a]);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
                o[tail + 4 + a] = __float_as_uint(__fmul_rn(__fdiv_rn(__fsub_rn((float)t[a], 32767.5f), 32767.5f), 1.41421356f));
            colour = lds_u32(in32, q + 20);
            sh_q = q + 24;
        }
        o[3] = o[4] = o[5] = 0u;                                   // normals: np.zeros
        o[6] = __float_as_uint(tab[colour & 0xffu]);
        o[7] = __float_as_uint(tab[(colour >> 8) & 0xffu]);
        o[8] = __float_as_uint(tab[(colour >> 16) & 0xffu]);
        o[tail] = __float_as_uint(tab[256 + (colour >> 24)]);
        for (int k = 0; k < A.sh_count; ++k) {
            unsigned v;
            if (LV == 0) v = lds_u32(in32, sh_q + 4 * k);
            else if (LV == 1) v = half_bits(lds_u32(in32, sh_q + 2 * k) & 0xffffu);
            else v = __float_as_uint(__fmul_rn((float)((int)(lds_u32(in32, sh_q + k) & 0xffu) - 128), 0.0078125f));
            o[rest + k] = v;
        }
        for (int k = A.sh_count; k < A.n_coeffs; ++k) o[rest + k] = 0u;
    }
    __syncthreads();
    store_words(out, gw0, cnt * A.row_words, o32, pad);
}

static size_t ksr_out_bytes(int row_words) { return (((size_t)KSR_TILE * row_words + 3 + 3) * 4 + 15) / 16 * 16; }

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_ksplat_unpack_dev(gsx_ctx *c, const void *body_dev, int64_t body_bytes, int level, const gsx_ksplat_read_section *sections,
                          int n_sections, const uint32_t *prefix_dev, int64_t n_prefix, const float *tables_dev, int n_coeffs, float *out_dev,
                          int64_t out_rows)
{
    if (!c || (n_sections > 0 && !sections)) GSX_FAIL("gsx_ksplat_unpack_dev: null argument");
    if (level < 0 || n_sections < 0 || body_bytes < 0 || n_prefix < 0 || out_rows < 0 || out_rows >= (1LL << 40))
        GSX_FAIL("gsx_ksplat_unpack_dev: bad level, section count or sizes");
    if (n_coeffs != 0 && n_coeffs != 9 && n_coeffs != 24 && n_coeffs != 45)
        GSX_FAIL("gsx_ksplat_unpack_dev: %d f_rest fields per output row (0, 9, 24 and 45 are supported)", n_coeffs);
    if ((reinterpret_cast<uintptr_t>(body_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15) || (reinterpret_cast<uintptr_t>(prefix_dev) & 3)
        || (reinterpret_cast<uintptr_t>(tables_dev) & 3))
        GSX_FAIL("gsx_ksplat_unpack_dev: body and output must be 16-byte aligned, prefix sums and tables 4-byte aligned");
    const int sh_item = level == 0 ? 4 : (level == 1 ? 2 : 1);
    // every section is checked before the first launch
    std::vector<KsReadArgs> args;
    for (int s = 0; s < n_sections; ++s) {
        const gsx_ksplat_read_section &S = sections[s];
        if (S.n_rows < 0 || S.n_rows >= (1LL << 32) || S.out_row < 0 || S.out_row + S.n_rows > out_rows)
            GSX_FAIL("gsx_ksplat_unpack_dev: section %d: rows [%lld, +%lld) of %lld output rows", s, (long long)S.out_row, (long long)S.n_rows,
                     (long long)out_rows);
        if (S.n_rows == 0) continue;
        if (!body_dev || !tables_dev || !out_dev) GSX_FAIL("gsx_ksplat_unpack_dev: null argument");
        if ((S.sh_count != 0 && S.sh_count != 9 && S.sh_count != 24) || S.sh_count > n_coeffs)
            GSX_FAIL("gsx_ksplat_unpack_dev: section %d: sh_count %d for %d f_rest fields", s, S.sh_count, n_coeffs);
        KsReadArgs A;
        A.row_bytes = (level == 0 ? 44 : 24) + sh_item * S.sh_count;
        if (S.rows_offset < 0 || S.rows_offset > body_bytes || S.n_rows > (body_bytes - S.rows_offset) / A.row_bytes)
            GSX_FAIL("gsx_ksplat_unpack_dev: section %d: %lld rows of %d bytes at %lld do not fit %lld body bytes", s, (long long)S.n_rows,
                     A.row_bytes, (long long)S.rows_offset, (long long)body_bytes);
        if (level >= 1) {
            if (S.n_buckets == 0 || S.centres_offset < 0 || S.centres_offset > body_bytes
                || (int64_t)S.n_buckets > (body_bytes - S.centres_offset) / 12)
                GSX_FAIL("gsx_ksplat_unpack_dev: section %d: %u bucket centres at %lld do not fit %lld body bytes", s, S.n_buckets,
                         (long long)S.centres_offset, (long long)body_bytes);
            if (S.full_rows < 0 || (S.full_rows > 0 && S.bucket_size == 0) || S.n_partial >= (1u << 31) || S.prefix_offset < 0
                || S.prefix_offset + (int64_t)S.n_partial > n_prefix || (S.n_partial > 0 && !prefix_dev))
                GSX_FAIL("gsx_ksplat_unpack_dev: section %d: bad bucket description", s);
            if (S.full_rows < S.n_rows && S.n_partial == 0)
                GSX_FAIL("gsx_ksplat_unpack_dev: section %d: the buckets cover %lld of %lld rows", s, (long long)S.full_rows, (long long)S.n_rows);
        }
        A.rows_off = S.rows_offset;
        A.cen_off = S.centres_offset;
        A.n = S.n_rows;
        A.out_row = S.out_row;
        A.full_rows = level >= 1 ? S.full_rows : 0;
        A.prefix_off = level >= 1 && S.n_partial ? S.prefix_offset : 0;
        A.bucket_size = S.bucket_size;
        A.n_full = S.n_full;
        A.n_partial = level >= 1 ? S.n_partial : 0;
        A.n_buckets = S.n_buckets;
        A.sh_count = S.sh_count;
        A.row_words = KSR_BASE + n_coeffs;
        A.n_coeffs = n_coeffs;
        A.in_quads = (int)(spz_in_bytes(KSR_TILE, A.row_bytes) / 16);
        A.sr = S.scale_range;
        A.sf = S.scale_factor;
        args.push_back(A);
    }
    GSX_HIP(hipSetDevice(c->device));
    for (const KsReadArgs &A : args) {
        const unsigned tiles = (unsigned)((A.n + KSR_TILE - 1) / KSR_TILE);
        const size_t lds = (size_t)A.in_quads * 16 + ksr_out_bytes(A.row_words);
        const uint4 *body = static_cast<const uint4 *>(body_dev);
        unsigned *out = reinterpret_cast<unsigned *>(out_dev);
        if (level == 0) hipLaunchKernelGGL(ksplat_unpack_kernel<0>, dim3(tiles), dim3(KSR_TILE), lds, c->stream, body, A, prefix_dev, tables_dev, out);
        else if (level == 1) hipLaunchKernelGGL(ksplat_unpack_kernel<1>, dim3(tiles), dim3(KSR_TILE), lds, c->stream, body, A, prefix_dev, tables_dev, out);
        else hipLaunchKernelGGL(ksplat_unpack_kernel<2>, dim3(tiles), dim3(KSR_TILE), lds, c->stream, body, A, prefix_dev, tables_dev, out);
        GSX_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
