// resident_rows.hip -- what a conversion does with a reader's decoded rows while they are still in HBM:
//
//   gsx_rows_columns_f32_dev  up to four 4-byte fields of every row as a dense (n, m) array of words: the chain's (n, 3)
//                             coordinates (data_processor.py:38,139), the alpha filter's opacity column (:210), the colours' f_dc
//   gsx_rows_take_dev         the device twin of csrc/host_rows.hip's gsx_host_take_rows_shape: `vertices[mask]` (:114,149),
//                             cap_sh_degree's column fill (:310-313) and add_rgb_from_sh's widened copy (:262-274) in one pass
//   gsx_dev_patch_u8          a few listed bytes of a device array set from host values (the colours numpy decides)
//
// Both row kernels take rows_dev as gsx_table_profile_dev does: a 16-byte aligned base, row 0 at byte 0 ... 15, 15 readable bytes
// past the last row, rows of 1 ... 512 bytes with fields at any byte offset.  The tile staging and the 16-byte stores are
// row_tile.h's.  Every value is a bit copy; every store is a plain vector store, and no two workgroups write the same byte.
#include <algorithm>

#include "row_tile.h"

namespace gsx {

struct ColumnOffsets {
    int off[4];
};

// one lane per row of a staged tile; blockDim.x = spz_tile_rows(rb).  The tile's m * cnt words are assembled in LDS and leave
// as whole quads (a tile starts at a multiple of 4 words: pad is 0, the last tile's tail is the ragged end)
__global__ void rows_columns_kernel(const uint4 *__restrict__ rows, int rb, int64_t first, int64_t n, ColumnOffsets O, int m,
                                    unsigned *__restrict__ out)
{
    extern __shared__ uint4 rc_lds[];
    const int tr = blockDim.x;
    const unsigned *in32 = reinterpret_cast<const unsigned *>(rc_lds);
    unsigned *o32 = reinterpret_cast<unsigned *>(rc_lds) + spz_in_bytes(tr, rb) / 4;
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();
        const int base = spz_stage_tile(rows, rb, t0, cnt, rc_lds, first);
        __syncthreads();
        const int64_t gw0 = t0 * m;
        const int pad = (int)(gw0 & 3);
        if ((int)threadIdx.x < cnt) {
            const int q = base + (int)threadIdx.x * rb;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < m) o32[pad + (int)threadIdx.x * m + j] = lds_u32(in32, q + O.off[j]);
        }
        __syncthreads();
        store_words(out, gw0, cnt * m, o32, pad);
    }
}

// The take kernel's tile is a quarter of the format kernels' (32 output rows, 16 above 256 bytes) and its workgroup two waves:
// a tile's life is a chain of memory latencies -- the index, the row's appended bytes, the source rows, the stores -- and with a
// staged input AND an output image of 32 KiB each only two workgroups fit a CU, which left HBM idle (10M rows of 248 bytes: 6.3 ms,
// six profile passes).  At 17 KiB of LDS a CU holds eight workgroups, and every lane's loads of a tile are issued before the first
// of them is stored to LDS.
constexpr int TAKE_THREADS = 128;
constexpr int TAKE_BATCH = 4;            // 16-byte loads a lane has in flight
static inline int take_tile_rows(int stride_out) { return spz_tile_rows(stride_out) / 4; }

constexpr size_t TAKE_MAX_LDS = 64 * 1024;   // (the default limit of dynamic LDS; the widest tile takes 17 KiB)

struct TakeArgs {
    int stride_in, stride_out, e, tile_rows;
    int slot_quads;          // quads that hold one source row from the 16-byte boundary at or below its first byte
    int in_bytes;            // LDS bytes of the staged source rows
    unsigned zero_bits[SPZ_MAX_ROW_BYTES / 32];   // bit b: byte b of a row is zeroed
};

// LDS bytes of the staged source rows: a contiguous run (spz_stage_tile) or a slot per row, whichever is larger
static inline size_t take_in_bytes(int tr, int stride_in)
{
    const size_t slots = (size_t)tr * ((stride_in + 15 + 15) / 16) * 16 + 16;
    return std::max(slots, spz_in_bytes(tr, stride_in));
}

// One workgroup per tile of OUTPUT rows [j0, j0 + cnt) (take_tile_rows).  Source row idx[j] is read whole with 16-byte loads -- the
// whole tile as one span when its source rows are consecutive (no filter, or a surviving run), a slot per row otherwise --, the tile's output
// image is assembled in LDS word by word (a word inside one row's copied bytes is one unaligned LDS read and a mask; a word that
// crosses into the appended bytes or the next row is put together byte by byte) and leaves through store_bytes.
// *bad is set when the list leaves [0, n_in) or does not ascend: such a row is read from row 0 and the caller discards the result.
__global__ __launch_bounds__(TAKE_THREADS) void rows_take_kernel(const uint4 *__restrict__ rows, int64_t first, int64_t n_in,
                                                                 const unsigned *__restrict__ idx, int64_t n_out,
                                                                 const unsigned char *__restrict__ extra, TakeArgs A,
                                                                 unsigned char *__restrict__ out, unsigned *__restrict__ bad)
{
    extern __shared__ uint4 tk_lds[];
    __shared__ int s_pos[32];                  // LDS byte of output row r's source row (take_tile_rows <= 32)
    __shared__ unsigned s_src[32];             // its index in the source table
    __shared__ unsigned s_extra[32];           // its appended bytes
    __shared__ unsigned s_zero[SPZ_MAX_ROW_BYTES / 32];
    __shared__ int s_run;                      // the tile's source rows are consecutive
    const int t = threadIdx.x;
    const int tr = A.tile_rows, si = A.stride_in, so = A.stride_out, e = A.e;
    const int64_t j0 = (int64_t)blockIdx.x * tr;
    const int cnt = (int)min((int64_t)tr, n_out - j0);
    const unsigned *in32 = reinterpret_cast<const unsigned *>(tk_lds);
    unsigned *img32 = reinterpret_cast<unsigned *>(tk_lds) + A.in_bytes / 4;
    if (t < SPZ_MAX_ROW_BYTES / 32) s_zero[t] = A.zero_bits[t];
    if (t < cnt) {
        const int64_t j = j0 + t;
        unsigned r = idx ? idx[j] : (unsigned)j;
        if ((int64_t)r >= n_in || (idx && j > 0 && idx[j - 1] >= r)) {
            *bad = 1u;
            r = 0u;
        }
        s_src[t] = r;
        unsigned x = 0u;
        for (int k = 0; k < e; ++k) x |= (unsigned)extra[(int64_t)r * e + k] << (8 * k);
        s_extra[t] = x;
    }
    __syncthreads();
    if (t == 0) s_run = s_src[cnt - 1] - s_src[0] == (unsigned)(cnt - 1);
    __syncthreads();
    if (s_run) {                               // (ascending and distinct: first and last cnt - 1 apart means consecutive)
        const int64_t b0 = first + (int64_t)s_src[0] * si, b1 = b0 + (int64_t)cnt * si;   // (spz_stage_tile's span)
        stage_span<TAKE_THREADS, TAKE_BATCH>(rows, b0 >> 4, (int)(((b1 + 15) >> 4) - (b0 >> 4)), tk_lds);
        if (t < cnt) s_pos[t] = (int)(b0 & 15) + t * si;
    } else {
        const int sq = A.slot_quads;
        for (int k0 = t; k0 < cnt * sq; k0 += TAKE_BATCH * TAKE_THREADS) {
            uint4 v[TAKE_BATCH];
            bool on[TAKE_BATCH];
#pragma unroll
            for (int u = 0; u < TAKE_BATCH; ++u) {
                const int k = k0 + u * TAKE_THREADS;
                on[u] = false;
                if (k < cnt * sq) {
                    const int r = k / sq, q = k - r * sq;
                    const int64_t b0 = first + (int64_t)s_src[r] * si;
                    on[u] = q < (int)(((b0 + si + 15) >> 4) - (b0 >> 4));
                    if (on[u]) v[u] = rows[(b0 >> 4) + q];
                }
            }
#pragma unroll
            for (int u = 0; u < TAKE_BATCH; ++u)
                if (on[u]) tk_lds[k0 + u * TAKE_THREADS] = v[u];
        }
        if (t < cnt) s_pos[t] = t * sq * 16 + (int)((first + (int64_t)s_src[t] * si) & 15);
    }
    __syncthreads();
    const int bytes = cnt * so, words = (bytes + 3) >> 2;
    const float inv = 1.0f / (float)so;
    for (int w = t; w < words; w += TAKE_THREADS) {
        const int p = 4 * w;
        int r = (int)((float)p * inv);         // p / so: the estimate is off by one at most
        r -= r * so > p;
        r += (r + 1) * so <= p;
        const int b = p - r * so;
        unsigned v;
        if (b + 4 <= si) {
            v = lds_u32(in32, s_pos[r] + b);
            // the zero bits of bytes b ... b + 3 (b <= 508: word (b >> 5) + 1 exists whenever the four bits cross into it)
            const unsigned z = (s_zero[b >> 5] >> (b & 31)) | (((b & 31) > 28) ? s_zero[(b >> 5) + 1] << (32 - (b & 31)) : 0u);
            if (z & 15u) v &= ~(((z & 1u) ? 0xffu : 0u) | ((z & 2u) ? 0xff00u : 0u) | ((z & 4u) ? 0xff0000u : 0u) | ((z & 8u) ? 0xff000000u : 0u));
        } else {
            v = 0u;
            int rr = r, bb = b;
            for (int k = 0; k < 4 && p + k < bytes; ++k) {
                unsigned byte;
                if (bb < si) byte = ((s_zero[bb >> 5] >> (bb & 31)) & 1u) ? 0u : lds_u8(in32, s_pos[rr] + bb);
                else byte = (s_extra[rr] >> (8 * (bb - si))) & 0xffu;
                v |= byte << (8 * k);
                if (++bb == so) {
                    bb = 0;
                    ++rr;
                }
            }
        }
        img32[w] = v;
    }
    __syncthreads();
    store_bytes(out, j0 * so, j0 * so + bytes, reinterpret_cast<const unsigned char *>(img32));
}

__global__ __launch_bounds__(256) void patch_u8_kernel(unsigned char *__restrict__ dst, int64_t dst_len, const unsigned *__restrict__ idx,
                                                       const unsigned char *__restrict__ val, int64_t cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt && (int64_t)idx[i] < dst_len) dst[idx[i]] = val[i];
}

}  // namespace gsx

using namespace gsx;

extern "C" int gsx_rows_columns_f32_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n, const int32_t *offsets,
                                        int m, void *out_dev)
{
    if (!c || !offsets || (n > 0 && (!rows_dev || !out_dev))) GSX_FAIL("gsx_rows_columns_f32_dev: null argument");
    if (n < 0 || n >= (1LL << 32) || m < 1 || m > 4) GSX_FAIL("gsx_rows_columns_f32_dev: %lld rows, %d columns (1 ... 4)", (long long)n, m);
    GSX_CHECK(rows_args(rows_dev, first_byte, stride, "gsx_rows_columns_f32_dev"));
    if (reinterpret_cast<uintptr_t>(out_dev) & 15) GSX_FAIL("gsx_rows_columns_f32_dev: the output must be 16-byte aligned");
    ColumnOffsets O = {{0, 0, 0, 0}};
    for (int j = 0; j < m; ++j) {
        if (offsets[j] < 0 || offsets[j] + 4 > stride) GSX_FAIL("gsx_rows_columns_f32_dev: column %d at byte offset %d of a %lld-byte row", j, offsets[j], (long long)stride);
        O.off[j] = offsets[j];
    }
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    const int rb = (int)stride, tr = spz_tile_rows(rb);
    const size_t lds = spz_in_bytes(tr, rb) + (size_t)tr * 16 + 16;
    hipLaunchKernelGGL(rows_columns_kernel, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), lds, c->stream, static_cast<const uint4 *>(rows_dev), rb,
                       first_byte, n, O, m, static_cast<unsigned *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

extern "C" int gsx_rows_take_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride_in, int64_t n_in, const uint32_t *idx_dev,
                                 int64_t n_out, const int32_t *zero_offsets, int n_zero, const uint8_t *extra_dev, int e, void *out_dev,
                                 int64_t stride_out)
{
    if (!c || (n_out > 0 && (!rows_dev || !out_dev)) || (n_zero > 0 && !zero_offsets) || (e > 0 && n_out > 0 && !extra_dev))
        GSX_FAIL("gsx_rows_take_dev: null argument");
    if (n_in < 0 || n_in >= (1LL << 32) || n_out < 0 || n_out > n_in || e < 0 || e > 4 || n_zero < 0 || n_zero > SPZ_MAX_ROW_BYTES / 4)
        GSX_FAIL("gsx_rows_take_dev: %lld of %lld rows, %d appended bytes (0 ... 4), %d zeroed fields", (long long)n_out, (long long)n_in, e, n_zero);
    GSX_CHECK(rows_args(rows_dev, first_byte, stride_in, "gsx_rows_take_dev"));
    if (stride_out != stride_in + e) GSX_FAIL("gsx_rows_take_dev: output rows of %lld bytes for %lld + %d", (long long)stride_out, (long long)stride_in, e);
    if (reinterpret_cast<uintptr_t>(out_dev) & 15) GSX_FAIL("gsx_rows_take_dev: the output must be 16-byte aligned");
    TakeArgs A;
    memset(&A, 0, sizeof(A));
    for (int k = 0; k < n_zero; ++k) {
        const int o = zero_offsets[k];
        if (o < 0 || o + 4 > stride_in) GSX_FAIL("gsx_rows_take_dev: zeroed field %d at byte offset %d of a %lld-byte row", k, o, (long long)stride_in);
        for (int b = o; b < o + 4; ++b) A.zero_bits[b >> 5] |= 1u << (b & 31);
    }
    GSX_HIP(hipSetDevice(c->device));
    if (n_out == 0) return 0;
    A.stride_in = (int)stride_in;
    A.stride_out = (int)stride_out;
    A.e = e;
    A.tile_rows = take_tile_rows((int)stride_out);
    A.slot_quads = ((int)stride_in + 15 + 15) / 16;
    A.in_bytes = (int)take_in_bytes(A.tile_rows, A.stride_in);
    const size_t lds = (size_t)A.in_bytes + ((size_t)A.tile_rows * A.stride_out + 32 + 15) / 16 * 16;   // + what store_bytes reads behind the image
    if (lds > TAKE_MAX_LDS) GSX_FAIL("gsx_rows_take_dev: a tile of %zu LDS bytes", lds);
    GSX_CHECK(c->nzmask.reserve(16));
    unsigned *d_bad = c->nzmask.as<unsigned>();
    GSX_HIP(hipMemsetAsync(d_bad, 0, 4, c->stream));
    const int64_t tiles = (n_out + A.tile_rows - 1) / A.tile_rows;
    hipLaunchKernelGGL(rows_take_kernel, dim3((unsigned)tiles), dim3(TAKE_THREADS), lds, c->stream, static_cast<const uint4 *>(rows_dev), first_byte,
                       n_in, idx_dev, n_out, extra_dev, A, static_cast<unsigned char *>(out_dev), d_bad);
    GSX_HIP(hipGetLastError());
    unsigned bad = 0;
    GSX_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if (bad) GSX_FAIL("gsx_rows_take_dev: the index list is not strictly ascending inside [0, n)");
    return 0;
}

extern "C" int gsx_dev_patch_u8(gsx_ctx *c, uint8_t *dst_dev, int64_t dst_len, const uint32_t *idx, const uint8_t *val, int64_t cnt)
{
    if (!c || (cnt > 0 && (!dst_dev || !idx || !val))) GSX_FAIL("gsx_dev_patch_u8: null argument");
    if (cnt < 0 || cnt >= (1LL << 31) || dst_len < 0) GSX_FAIL("gsx_dev_patch_u8: %lld entries for %lld bytes", (long long)cnt, (long long)dst_len);
    for (int64_t i = 0; i < cnt; ++i)
        if ((int64_t)idx[i] >= dst_len) GSX_FAIL("gsx_dev_patch_u8: entry %lld at byte %u of %lld", (long long)i, idx[i], (long long)dst_len);
    GSX_HIP(hipSetDevice(c->device));
    if (cnt == 0) return 0;
    unsigned *d_idx = nullptr;
    unsigned char *d_val = nullptr;
    GSX_CHECK(carve(c->work, [&](Carve &a) {
        d_idx = a.take<unsigned>((size_t)cnt);
        d_val = a.take<unsigned char>((size_t)cnt, 16);
    }));
    GSX_HIP(hipMemcpyAsync(d_idx, idx, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(hipMemcpyAsync(d_val, val, (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(patch_u8_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, c->stream, dst_dev, dst_len, d_idx, d_val, cnt);
    GSX_HIP(hipGetLastError());
    GSX_HIP(hipStreamSynchronize(c->stream));   // (the host arrays are the caller's again)
    return 0;
}
