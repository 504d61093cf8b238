// ply_text.hip -- the body of an ASCII PLY element -> its rows in binary little-endian form, as gsx_ply_unpack_dev expects them.
//
// Replaces, for a file of `format ascii 1.0`, what gsconverter/formats/ply_3dgs.py:10 and gsconverter/formats/ply_cc.py:10
// (PlyData.read) get from plyfile: one Python call per value there, one pass over the text here.  The contract (DESIGN.md,
// "ASCII PLY bodies") is the intersection of what the two generations of plyfile return:
//   lines    end at \n; tokens are separated by runs of 0x20 0x09 0x0b 0x0c 0x0d; every line of the element holds exactly as many
//            tokens as the element has properties
//   float    the grammar and the certified rounding of dec_to_f64.h; `float` is that double cast to float32 (rounded twice, as
//            numpy does)
//   integer  [+-]?D+ within the property's range
// A chunk of text starts at a line start and ends with a newline.  Three kernels:
//   scan     a workgroup per tile of 4096 bytes, 16 bytes a lane: token starts (a non-blank byte behind a blank one) and newlines
//            are counted per tile
//   prefix   one workgroup: the exclusive scan of the tile counts, the totals
//   parse    a workgroup per tile again: the token starts are compacted into LDS and the lanes take tokens densely; token t of
//            the chunk is row t / P, column t % P -- valid because every newline j checks that (j + 1) P tokens precede it, and
//            the first line that breaks the rule is recorded (atomicMin).  A token the lane cannot settle (not of the grammar,
//            out of range, uncertified, a subnormal result, longer than TXT_CAP bytes) is listed for the host and its bytes stay
//            zero; the host patches them (the pattern of gsx_dev_patch_u8) or refuses the file.
// gsx_ply_text_host is the same tokeniser and the same number code on a host buffer: the host tests' model, and what converts
// a chunk whose list overflowed.
#include <algorithm>

#include "dec_to_f64.h"
#include "gsx_common.h"
#include "row_tile.h"

namespace gsx {

constexpr int TXT_THREADS = 256;
constexpr int TXT_TILE = 16 * TXT_THREADS;    // bytes of text per workgroup
constexpr int TXT_LOOK = 64;                  // bytes staged behind the tile: a token that starts in the tile is walked in LDS
constexpr int TXT_CAP = 63;                   // the longest token a lane parses
constexpr int TXT_MAX_PROPS = GSX_PLY_TEXT_MAX_PROPS;
constexpr int64_t TXT_MAX_LEN = (int64_t)1 << 30;
enum { TXT_R_TOKENS = 0, TXT_R_LINES, TXT_R_ERR, TXT_R_FLAGGED, TXT_R_END, TXT_R_WORDS = 16 };

struct PlyTextArgs {
    int n_props, in_stride;
    unsigned short desc[TXT_MAX_PROPS];       // byte offset inside a row (10 bits) | GSX_PLY_T_* << 10
};

__host__ __device__ inline bool txt_newline(unsigned c) { return c == 0x0au; }
// a separator, or the newline (which ends a token as well)
__host__ __device__ inline bool txt_blank(unsigned c) { return c == 0x20u || (c - 9u) < 5u; }

__host__ __device__ inline int txt_type_bytes(unsigned type) { return type <= GSX_PLY_T_U1 ? 1 : type <= GSX_PLY_T_U2 ? 2 : type <= GSX_PLY_T_F4 ? 4 : 8; }

// one token of n bytes and of property type `type` -> the little-endian bytes of its value in *value (DEC_OK), or DEC_FLAG
template <class B>
__host__ __device__ inline int txt_value(const B &byte, int n, unsigned type, uint64_t *value)
{
    if (type == GSX_PLY_T_F8) return dec_to_f64(byte, n, value);
    if (type == GSX_PLY_T_F4) {
        uint64_t b;
        if (dec_to_f64(byte, n, &b) != DEC_OK) return DEC_FLAG;
        *value = ply_f64_to_f32((unsigned)b, (unsigned)(b >> 32));
        return DEC_OK;
    }
    int64_t lo, hi, v;
    switch (type) {
    case GSX_PLY_T_I1: lo = -128, hi = 127; break;
    case GSX_PLY_T_U1: lo = 0, hi = 255; break;
    case GSX_PLY_T_I2: lo = -32768, hi = 32767; break;
    case GSX_PLY_T_U2: lo = 0, hi = 65535; break;
    case GSX_PLY_T_I4: lo = -2147483648LL, hi = 2147483647LL; break;
    default: lo = 0, hi = 4294967295LL; break;
    }
    if (dec_to_int(byte, n, lo, hi, &v) != DEC_OK) return DEC_FLAG;
    *value = (uint64_t)v;
    return DEC_OK;
}

// the lane's 16 bytes at byte b0 of the chunk, `prev` the byte before them -> bit i of tok: byte i starts a token; of nl: byte i
// is a newline.  Bytes at or past `len` count as nothing.
__device__ __forceinline__ void txt_classify(const uint4 v, unsigned prev, unsigned b0, unsigned len, unsigned &tok, unsigned &nl)
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    tok = nl = 0u;
    bool before = txt_blank(prev);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool blank = txt_blank(c), live = b0 + i < len;
        if (live && !blank && before) tok |= 1u << i;
        if (live && txt_newline(c)) nl |= 1u << i;
        before = blank;
    }
}

__device__ __forceinline__ unsigned txt_prev_byte(const uint4 *__restrict__ text, unsigned b0)
{
    return b0 ? reinterpret_cast<const unsigned char *>(text)[b0 - 1] : 0x0au;
}

// packed counts (token starts | newlines << 16) of the workgroup's lanes -> each lane's exclusive prefix, *total
__device__ __forceinline__ unsigned txt_block_scan(unsigned v, unsigned *total, unsigned *wsum /*[4]*/)
{
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(inc, off);
        if ((int)(threadIdx.x & 63) >= off) inc += o;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned s = wsum[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    __syncthreads();
    return base + inc - v;
}

// text: the chunk from its first byte, 16-byte aligned, readable up to tiles * TXT_TILE + TXT_LOOK bytes
__global__ __launch_bounds__(TXT_THREADS) void ply_text_scan_kernel(const uint4 *__restrict__ text, unsigned len, uint2 *__restrict__ tile_cnt)
{
    __shared__ unsigned s_w[4];
    const unsigned b0 = blockIdx.x * TXT_TILE + threadIdx.x * 16;
    unsigned tok, nl;
    txt_classify(text[b0 >> 4], txt_prev_byte(text, b0), b0, len, tok, nl);
    unsigned total;
    (void)txt_block_scan(__popc(tok) | (__popc(nl) << 16), &total, s_w);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = make_uint2(total & 0xffffu, total >> 16);
}

// exclusive scan of the tile counts in place (one workgroup); the totals -> tile_cnt[ntiles] and res, whose other words are reset
__global__ __launch_bounds__(1024) void ply_text_prefix_kernel(uint2 *__restrict__ tile_cnt, int ntiles, unsigned *__restrict__ res)
{
    __shared__ unsigned s_a[16], s_b[16];
    __shared__ unsigned s_ca, s_cb;
    if (threadIdx.x == 0) s_ca = s_cb = 0;
    __syncthreads();
    for (int b = 0; b < ntiles; b += 1024) {
        const int i = b + threadIdx.x;
        const uint2 v = i < ntiles ? tile_cnt[i] : make_uint2(0u, 0u);
        unsigned ia = v.x, ib = v.y;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned oa = __shfl_up(ia, off), ob = __shfl_up(ib, off);
            if ((int)(threadIdx.x & 63) >= off) {
                ia += oa;
                ib += ob;
            }
        }
        if ((threadIdx.x & 63) == 63) {
            s_a[threadIdx.x >> 6] = ia;
            s_b[threadIdx.x >> 6] = ib;
        }
        __syncthreads();
        unsigned pa = s_ca, pb = s_cb;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) {
            pa += s_a[w];
            pb += s_b[w];
        }
        if (i < ntiles) tile_cnt[i] = make_uint2(pa + ia - v.x, pb + ib - v.y);
        __syncthreads();
        if (threadIdx.x == 1023) {
            s_ca = pa + ia;
            s_cb = pb + ib;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tile_cnt[ntiles] = make_uint2(s_ca, s_cb);
        res[TXT_R_TOKENS] = s_ca;
        res[TXT_R_LINES] = s_cb;
        res[TXT_R_ERR] = 0xffffffffu;
        res[TXT_R_FLAGGED] = 0u;
        res[TXT_R_END] = 0u;
    }
}

struct TxtLdsByte {
    const unsigned *lds;
    int at;
    __device__ __forceinline__ unsigned operator()(int i) const { return lds_u8(lds, at + i); }
};

// `value`'s low nb bytes -> dst (any alignment)
__device__ __forceinline__ void txt_store(unsigned char *__restrict__ dst, uint64_t value, int nb)
{
    if (nb == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<unsigned *>(dst) = (unsigned)value;
    } else if (nb == 8 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
        *reinterpret_cast<unsigned long long *>(dst) = value;
    } else {
        for (int i = 0; i < nb; ++i) dst[i] = (unsigned char)(value >> (8 * i));
    }
}

// tile_pre: ply_text_prefix_kernel's; rows_left: rows the element still lacks (>= 1) -- the chunk's first min(rows_left, lines)
// lines are rows, written from rows_out on.  list: (token of the chunk, its byte offset, its length or 0 beyond TXT_CAP, 0)
__global__ __launch_bounds__(TXT_THREADS) void ply_text_parse_kernel(const uint4 *__restrict__ text, unsigned len, const uint2 *__restrict__ tile_pre,
                                                                     int ntiles, unsigned rows_left, PlyTextArgs A, unsigned char *__restrict__ rows_out,
                                                                     unsigned *__restrict__ res, uint4 *__restrict__ list, unsigned list_cap)
{
    __shared__ uint4 s_text[(TXT_TILE + TXT_LOOK) / 16];
    __shared__ unsigned short s_pos[TXT_TILE / 2 + 1];     // a token start needs a blank byte before it: at most TXT_TILE / 2 + 1 a tile
    __shared__ unsigned s_w[4];
    const unsigned tid = threadIdx.x, t0 = blockIdx.x * TXT_TILE, b0 = t0 + tid * 16;
    const uint4 v = text[b0 >> 4];
    s_text[tid] = v;
    if (tid < TXT_LOOK / 16) s_text[TXT_THREADS + tid] = text[(t0 >> 4) + TXT_THREADS + tid];
    unsigned tok, nl;
    txt_classify(v, txt_prev_byte(text, b0), b0, len, tok, nl);
    unsigned total;
    const unsigned ex = txt_block_scan(__popc(tok) | (__popc(nl) << 16), &total, s_w);   // (its barriers also publish s_text)
    const uint2 pre = tile_pre[blockIdx.x];
    const unsigned rows = min(rows_left, tile_pre[ntiles].y);
    const unsigned P = (unsigned)A.n_props;
    const uint64_t wanted = (uint64_t)rows * P;
    unsigned tk = ex & 0xffffu;
    for (unsigned m = tok; m; m &= m - 1) s_pos[tk++] = (unsigned short)(tid * 16 + (__ffs(m) - 1));
    unsigned line = pre.y + (ex >> 16);
    for (unsigned m = nl; m; m &= m - 1, ++line) {
        if (line >= rows) break;
        const unsigned k = __ffs(m) - 1;
        const uint64_t before = (uint64_t)pre.x + (ex & 0xffffu) + __popc(tok & ((1u << k) - 1u));
        if (before != (uint64_t)(line + 1) * P) atomicMin(&res[TXT_R_ERR], line);
        if (line == rows - 1) res[TXT_R_END] = b0 + k + 1;
    }
    __syncthreads();
    const unsigned ntok = total & 0xffffu;
    const unsigned *lds = reinterpret_cast<const unsigned *>(s_text);
    for (unsigned i = tid; i < ntok; i += TXT_THREADS) {
        const uint64_t t = (uint64_t)pre.x + i;
        if (t >= wanted) break;
        const unsigned row = (unsigned)t / P, col = (unsigned)t - row * P;     // (a chunk holds fewer than 2^31 tokens)
        const unsigned d = A.desc[col], type = d >> 10;
        const int at = s_pos[i], nb = txt_type_bytes(type);
        int n = 0;
        while (n <= TXT_CAP && !txt_blank(lds_u8(lds, at + n))) ++n;
        uint64_t value = 0;
        if (n > TXT_CAP || txt_value(TxtLdsByte{lds, at}, n, type, &value) != DEC_OK) {
            const unsigned k = atomicAdd(&res[TXT_R_FLAGGED], 1u);
            if (k < list_cap) list[k] = make_uint4((unsigned)t, t0 + at, n > TXT_CAP ? 0u : (unsigned)n, 0u);
            value = 0;
        }
        txt_store(rows_out + (size_t)row * A.in_stride + (d & 0x3ffu), value, nb);
    }
}

static int txt_layout_to_args(const gsx_ply_text_layout *l, PlyTextArgs *A, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (l->n_props < 1 || l->n_props > TXT_MAX_PROPS) GSX_FAIL("%s: %d properties (1 ... %d are supported)", who, l->n_props, TXT_MAX_PROPS);
    if (l->in_stride < 1 || l->in_stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("%s: rows of %d bytes (1 ... %d are supported)", who, l->in_stride, SPZ_MAX_ROW_BYTES);
    for (int p = 0; p < l->n_props; ++p) {
        const int type = l->type[p], off = l->offset[p];
        if (type < GSX_PLY_T_I1 || type > GSX_PLY_T_F8) GSX_FAIL("%s: property %d has type code %d", who, p, type);
        if (off < 0 || off + txt_type_bytes((unsigned)type) > l->in_stride)
            GSX_FAIL("%s: property %d of %d bytes at offset %d of a %d-byte row", who, p, txt_type_bytes((unsigned)type), off, l->in_stride);
        A->desc[p] = (unsigned short)((unsigned)off | ((unsigned)type << 10));
    }
    for (int p = l->n_props; p < TXT_MAX_PROPS; ++p) A->desc[p] = 0;
    A->n_props = l->n_props;
    A->in_stride = l->in_stride;
    return 0;
}

static int64_t txt_tiles(int64_t len) { return (len + TXT_TILE - 1) / TXT_TILE; }

static int txt_check_chunk(const void *text_dev, int64_t len, const void *work_dev, int64_t work_bytes, const char *who)
{
    if (!text_dev || !work_dev) GSX_FAIL("%s: null argument", who);
    if ((reinterpret_cast<uintptr_t>(text_dev) & 15) || (reinterpret_cast<uintptr_t>(work_dev) & 15)) GSX_FAIL("%s: text and work must be 16-byte aligned", who);
    if (len < 1 || len > TXT_MAX_LEN) GSX_FAIL("%s: a chunk of %lld bytes (1 ... %lld are supported)", who, (long long)len, (long long)TXT_MAX_LEN);
    if (work_bytes < gsx_ply_text_work_bytes(len)) GSX_FAIL("%s: work of %lld bytes, %lld are needed", who, (long long)work_bytes, (long long)gsx_ply_text_work_bytes(len));
    return 0;
}

struct TxtHostByte {
    const unsigned char *p;
    unsigned operator()(int i) const { return p[i]; }
};

}  // namespace gsx

using namespace gsx;

extern "C" {

int64_t gsx_ply_text_padded_bytes(int64_t text_len) { return text_len < 0 ? -1 : txt_tiles(text_len) * TXT_TILE + TXT_LOOK; }

int64_t gsx_ply_text_work_bytes(int64_t text_len) { return text_len < 0 ? -1 : 4 * TXT_R_WORDS + 8 * (txt_tiles(text_len) + 1); }

int gsx_ply_text_scan_dev(gsx_ctx *c, const void *text_dev, int64_t text_len, void *work_dev, int64_t work_bytes)
{
    if (!c) GSX_FAIL("gsx_ply_text_scan_dev: null argument");
    GSX_CHECK(txt_check_chunk(text_dev, text_len, work_dev, work_bytes, "gsx_ply_text_scan_dev"));
    const int tiles = (int)txt_tiles(text_len);
    unsigned *res = static_cast<unsigned *>(work_dev);
    uint2 *tile = reinterpret_cast<uint2 *>(res + TXT_R_WORDS);
    GSX_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(ply_text_scan_kernel, dim3(tiles), dim3(TXT_THREADS), 0, c->stream, static_cast<const uint4 *>(text_dev), (unsigned)text_len, tile);
    GSX_HIP(hipGetLastError());
    hipLaunchKernelGGL(ply_text_prefix_kernel, dim3(1), dim3(1024), 0, c->stream, tile, tiles, res);
    GSX_HIP(hipGetLastError());
    return 0;
}

int gsx_ply_text_parse_dev(gsx_ctx *c, const void *text_dev, int64_t text_len, int64_t rows_left, const gsx_ply_text_layout *layout,
                           void *rows_dev, void *work_dev, int64_t work_bytes, void *list_dev, int64_t list_cap, int64_t *result)
{
    if (!c || !result) GSX_FAIL("gsx_ply_text_parse_dev: null argument");
    PlyTextArgs A;
    GSX_CHECK(txt_layout_to_args(layout, &A, "gsx_ply_text_parse_dev"));
    GSX_CHECK(txt_check_chunk(text_dev, text_len, work_dev, work_bytes, "gsx_ply_text_parse_dev"));
    if (rows_left < 1 || !rows_dev || list_cap < 0 || list_cap > 0x7fffffff || (list_cap > 0 && !list_dev) || (reinterpret_cast<uintptr_t>(list_dev) & 15))
        GSX_FAIL("gsx_ply_text_parse_dev: bad arguments");
    const int tiles = (int)txt_tiles(text_len);
    unsigned *res = static_cast<unsigned *>(work_dev);
    const uint2 *tile = reinterpret_cast<const uint2 *>(res + TXT_R_WORDS);
    GSX_HIP(hipSetDevice(c->device));
    hipLaunchKernelGGL(ply_text_parse_kernel, dim3(tiles), dim3(TXT_THREADS), 0, c->stream, static_cast<const uint4 *>(text_dev), (unsigned)text_len, tile,
                       tiles, (unsigned)std::min<int64_t>(rows_left, 0x7fffffff), A, static_cast<unsigned char *>(rows_dev), res,
                       static_cast<uint4 *>(list_dev), (unsigned)list_cap);
    GSX_HIP(hipGetLastError());
    unsigned h[TXT_R_WORDS];
    GSX_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    result[GSX_PLY_TEXT_TOKENS] = h[TXT_R_TOKENS];
    result[GSX_PLY_TEXT_LINES] = h[TXT_R_LINES];
    result[GSX_PLY_TEXT_ROWS] = std::min<int64_t>(rows_left, h[TXT_R_LINES]);
    result[GSX_PLY_TEXT_BAD_LINE] = h[TXT_R_ERR] == 0xffffffffu ? -1 : (int64_t)h[TXT_R_ERR];
    result[GSX_PLY_TEXT_FLAGGED] = h[TXT_R_FLAGGED];
    result[GSX_PLY_TEXT_END] = h[TXT_R_END];
    return 0;
}

int gsx_ply_text_host(const void *text, int64_t text_len, int64_t rows_left, const gsx_ply_text_layout *layout, void *rows, uint32_t *list,
                      int64_t list_cap, int64_t *result)
{
    PlyTextArgs A;
    GSX_CHECK(txt_layout_to_args(layout, &A, "gsx_ply_text_host"));
    if (!text || !rows || !result || text_len < 1 || text_len > TXT_MAX_LEN || rows_left < 1 || list_cap < 0 || (list_cap > 0 && !list))
        GSX_FAIL("gsx_ply_text_host: bad arguments");
    const unsigned char *s = static_cast<const unsigned char *>(text);
    unsigned char *out = static_cast<unsigned char *>(rows);
    int64_t lines = 0;
    for (int64_t i = 0; i < text_len; ++i) lines += txt_newline(s[i]) ? 1 : 0;
    const int64_t n_rows = std::min(rows_left, lines), P = A.n_props, wanted = n_rows * P;
    int64_t tokens = 0, line = 0, bad = -1, flagged = 0, end = 0;
    bool before = true;   // (the chunk starts behind a newline)
    for (int64_t i = 0; i < text_len; ++i) {
        const unsigned ch = s[i];
        const bool blank = txt_blank(ch);
        if (!blank && before) {
            const int64_t t = tokens++;
            if (t < wanted) {
                int n = 0;
                while (n <= TXT_CAP && i + n < text_len && !txt_blank(s[i + n])) ++n;
                const int64_t row = t / P, col = t - row * P;
                const unsigned d = A.desc[col], type = d >> 10;
                uint64_t value = 0;
                if (n > TXT_CAP || txt_value(TxtHostByte{s + i}, n, type, &value) != DEC_OK) {
                    const int64_t k = flagged++;
                    if (k < list_cap) {
                        list[4 * k] = (uint32_t)t;
                        list[4 * k + 1] = (uint32_t)i;
                        list[4 * k + 2] = n > TXT_CAP ? 0u : (uint32_t)n;
                        list[4 * k + 3] = 0u;
                    }
                    value = 0;
                }
                unsigned char *dst = out + row * A.in_stride + (d & 0x3ffu);
                for (int b = 0; b < txt_type_bytes(type); ++b) dst[b] = (unsigned char)(value >> (8 * b));
            }
        }
        if (txt_newline(ch)) {
            if (line < n_rows) {
                if (tokens != (line + 1) * P && bad < 0) bad = line;
                if (line == n_rows - 1) end = i + 1;
            }
            ++line;
        }
        before = blank;
    }
    result[GSX_PLY_TEXT_TOKENS] = tokens;
    result[GSX_PLY_TEXT_LINES] = lines;
    result[GSX_PLY_TEXT_ROWS] = n_rows;
    result[GSX_PLY_TEXT_BAD_LINE] = bad;
    result[GSX_PLY_TEXT_FLAGGED] = flagged;
    result[GSX_PLY_TEXT_END] = end;
    return 0;
}

int gsx_dec_to_f64(const void *token, int32_t n, uint64_t *bits)
{
    if (!token || !bits || n < 0) GSX_FAIL("gsx_dec_to_f64: bad arguments");
    return dec_to_f64(TxtHostByte{static_cast<const unsigned char *>(token)}, n, bits) == DEC_OK ? 0 : GSX_DEC_FLAGGED;
}

int gsx_dec_pow5_entry(int32_t q, uint64_t *hi, uint64_t *lo, int32_t *exp2)
{
    if (q < GSX_DEC_QMIN || q > GSX_DEC_QMAX || !hi || !lo || !exp2) GSX_FAIL("gsx_dec_pow5_entry: q = %d (%d ... %d)", q, GSX_DEC_QMIN, GSX_DEC_QMAX);
    dec_pow5(q, *hi, *lo);
    *exp2 = dec_pow5_exp(q);
    return 0;
}

}  // extern "C"
