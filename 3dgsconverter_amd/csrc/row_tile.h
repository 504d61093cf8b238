// row_tile.h -- what the format kernels share: the writers that read a raw splat table in place (csrc/spz.hip, csrc/ksplat.hip,
// csrc/splat.hip, csrc/cply.hip, csrc/ply_write.hip) and the readers that decode a file's rows (csrc/cply_read.hip,
// csrc/ksplat_read.hip, csrc/spz_read.hip, csrc/sog_read.hip, csrc/splat_read.hip, csrc/ply_read.hip).  The f_rest scan of the
// SPZ, .ksplat and PLY writers has a header of its own beside this one (rest_scan.h).
//
// A workgroup owns a tile of consecutive rows: the tile's raw bytes are staged in LDS with 16-byte loads (any row size up to
// 512 bytes, fields at any byte offset: a field is assembled from two LDS words), and a tile's output leaves LDS as one
// contiguous span in 16-byte stores.  The layout is gsx_spz_layout's: float32 fields in gsx_sog_layout's order, -1 = absent.
// The float <-> integer keys live in sog_math.h (sort_key, float_key, sort_unkey).
#pragma once
#include <cstddef>

#include "gsx_common.h"

namespace gsx {

constexpr int SPZ_FIELDS = 59;   // x y z | rot_0..3 | scale_0..2 | f_dc_0..2 | opacity | f_rest_0..44 (gsx_sog_layout's order)
constexpr int SPZ_F_ROT = 3, SPZ_F_SCALE = 7, SPZ_F_DC = 10, SPZ_F_OPACITY = 13, SPZ_F_REST = 14;
constexpr int SPZ_MAX_ROW_BYTES = 512;

struct SpzLayoutDev {
    int row_bytes;
    int off[SPZ_FIELDS];   // byte offset inside a row, -1 = absent
};

// rows per tile (= threads per workgroup): the staged input stays within 32 KiB
static inline int spz_tile_rows(int row_bytes) { return row_bytes <= 256 ? 128 : 64; }

// LDS bytes of a tile: the staged rows (16-byte aligned window, one spare quad) + the output image (+16 spare bytes)
__host__ __device__ inline size_t spz_in_bytes(int tr, int row_bytes) { return ((size_t)tr * row_bytes + 15 + 15) / 16 * 16 + 16; }

// the little-endian u32 / float32 at any byte address of global memory: the two aligned words around it (reads at most 4
// bytes past the field)
__device__ __forceinline__ unsigned ld_u32(const unsigned char *__restrict__ base, int64_t byte)
{
    const unsigned *w = reinterpret_cast<const unsigned *>(base + (byte & ~(int64_t)3));
    return __builtin_amdgcn_alignbyte(w[1], w[0], (unsigned)(byte & 3));
}
__device__ __forceinline__ float ld_f32(const unsigned char *__restrict__ base, int64_t byte) { return __uint_as_float(ld_u32(base, byte)); }

// the little-endian u32 / float32 / byte at LDS byte index q (any alignment)
__device__ __forceinline__ unsigned lds_u32(const unsigned *lds, int q)
{
    return __builtin_amdgcn_alignbyte(lds[(q >> 2) + 1], lds[q >> 2], (unsigned)(q & 3));
}
__device__ __forceinline__ float lds_f32(const unsigned *lds, int q) { return __uint_as_float(lds_u32(lds, q)); }
__device__ __forceinline__ unsigned lds_u8(const unsigned *lds, int q) { return (lds[q >> 2] >> (8 * (q & 3))) & 0xffu; }

// numpy's float16 -> float32: exact, and a NaN keeps its sign, its payload and its quiet bit as they are (host and device: the
// host twins of the readers run it too)
__host__ __device__ __forceinline__ unsigned half_bits(unsigned h)
{
    if ((h & 0x7c00u) == 0x7c00u && (h & 0x03ffu)) return ((h & 0x8000u) << 16) | 0x7f800000u | ((h & 0x03ffu) << 13);
    union { unsigned short u; _Float16 f; } v;
    v.u = (unsigned short)h;
    const float f = (float)v.f;
    return __builtin_bit_cast(unsigned, f);
}

// float64 bits -> float32 bits: the plain cast.  On the host it is x86's cvtsd2ss, which numpy's cast runs; on the device it is
// v_cvt_f32_f64, which gives the same bits for every pattern tried (round to nearest even, overflow to +-inf, subnormal results
// kept, a NaN's sign and top payload bits kept, a signalling NaN quieted: DESIGN.md section 6j)
__host__ __device__ inline unsigned ply_f64_to_f32(unsigned lo, unsigned hi)
{
    const unsigned long long b = ((unsigned long long)hi << 32) | lo;
    const float f = (float)__builtin_bit_cast(double, b);
    return __builtin_bit_cast(unsigned, f);
}

// np.clip(t, 0, 255).astype(np.uint8): NaN stays NaN through the clip and casts to 0
__device__ __forceinline__ unsigned spz_u8(float t)
{
    return t == t ? (unsigned)fminf(fmaxf(t, 0.0f), 255.0f) : 0u;
}

// x86's float32 bits of a NaN result of two operands: the first NaN operand, quieted; an invalid operation of two numbers gives
// the negative default NaN (cold: only reached when the result is NaN, where the device's own NaN bits differ)
__device__ __noinline__ unsigned x86_nan(float first, float second)
{
    if (first != first) return __float_as_uint(first) | 0x00400000u;
    if (second != second) return __float_as_uint(second) | 0x00400000u;
    return 0xffc00000u;
}

// hand (idx, kind) to the host: the list keeps the first `cap` entries, *count counts them all
__device__ __forceinline__ void list_append(uint2 *list, unsigned cap, unsigned *count, unsigned idx, unsigned kind)
{
    const unsigned k = atomicAdd(count, 1u);
    if (k < cap) list[k] = make_uint2(idx, kind);
}

// rows [t0, t0 + cnt) of `row_bytes` bytes, row 0 at byte `first` of `rows` -> LDS, from the 16-byte boundary at or below the
// tile's first byte; -> that boundary's offset.  Reads at most 15 bytes past the last row (the caller's allocation has that slack).
__device__ __forceinline__ int spz_stage_tile(const uint4 *__restrict__ rows, int row_bytes, int64_t t0, int cnt, uint4 *lds, int64_t first = 0)
{
    const int64_t b0 = first + t0 * row_bytes, b1 = b0 + (int64_t)cnt * row_bytes;
    const int64_t q0 = b0 >> 4, q1 = (b1 + 15) >> 4;
    const int nq = (int)(q1 - q0);
    for (int k = threadIdx.x; k < nq; k += blockDim.x) lds[k] = rows[q0 + k];
    return (int)(b0 & 15);
}

// quads [q0, q0 + nq) of `rows` -> lds[0 .. nq) by a workgroup of THREADS lanes, BATCH 16-byte loads per lane in flight: every
// load of a round is issued before the first of them is stored to LDS (the resident-row kernels: csrc/resident_rows.hip,
// csrc/rows_remap.hip)
template <int THREADS, int BATCH>
__device__ __forceinline__ void stage_span(const uint4 *__restrict__ rows, int64_t q0, int nq, uint4 *lds)
{
    for (int k0 = threadIdx.x; k0 < nq; k0 += BATCH * THREADS) {
        uint4 v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) v[u] = rows[q0 + min(k0 + u * THREADS, nq - 1)];   // (no branch between the loads: past the end, the last quad again)
        // the loads stay above this line: without it the compiler sinks each of them into the branch of its store, where it is
        // issued, waited for and stored before the next one starts
#pragma unroll
        for (int u = 0; u < BATCH; ++u) asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w) : : "memory");
#pragma unroll
        for (int u = 0; u < BATCH; ++u)
            if (k0 + u * THREADS < nq) lds[k0 + u * THREADS] = v[u];
    }
}

// LDS image `img` -> bytes [g0, g1) of `out` (16-byte aligned), by the whole workgroup: bytes up to a 16-byte boundary, 16-byte
// stores assembled from the image's words (the image may start at any byte; up to 19 bytes behind it are read, never used),
// the tail bytes
__device__ __forceinline__ void store_bytes(unsigned char *__restrict__ out, int64_t g0, int64_t g1, const unsigned char *img)
{
    const int64_t h = min(g1, (g0 + 15) & ~(int64_t)15);
    const int64_t tl = max(h, g1 & ~(int64_t)15);
    const int nh = (int)(h - g0), nt = (int)(g1 - tl), nb = (int)((tl - h) >> 4);
    const int t = threadIdx.x;
    if (t < nh) out[g0 + t] = img[t];
    if (t < nt) out[tl + t] = img[(int)(tl - g0) + t];
    for (int k = t; k < nb; k += blockDim.x) {
        const int o = nh + 16 * k;                               // byte of the image that lands on the aligned address
        const unsigned *w32 = reinterpret_cast<const unsigned *>(img + (o & ~3));
        const unsigned sh = (unsigned)(o & 3);
        const unsigned a0 = w32[0], a1 = w32[1], a2 = w32[2], a3 = w32[3], a4 = w32[4];
        uint4 v;
        v.x = __builtin_amdgcn_alignbyte(a1, a0, sh);
        v.y = __builtin_amdgcn_alignbyte(a2, a1, sh);
        v.z = __builtin_amdgcn_alignbyte(a3, a2, sh);
        v.w = __builtin_amdgcn_alignbyte(a4, a3, sh);
        *reinterpret_cast<uint4 *>(out + h + 16 * k) = v;
    }
}

// `words` words at o32 + pad (o32 16-byte aligned in LDS, pad = gw0 & 3) -> words [gw0, gw0 + words) of `out` (16-byte aligned),
// by the whole workgroup: whole quads from LDS quad (q - (gw0 >> 2)), the ragged ends word by word
__device__ __forceinline__ void store_words(unsigned *__restrict__ out, int64_t gw0, int words, const unsigned *o32, int pad)
{
    const int64_t gw1 = gw0 + words;
    const int64_t qa = (gw0 + 3) >> 2, qb = gw1 >> 2, qz = gw0 >> 2;
    const uint4 *src = reinterpret_cast<const uint4 *>(o32);
    uint4 *dst = reinterpret_cast<uint4 *>(out);
    for (int64_t k = qa + threadIdx.x; k < qb; k += blockDim.x) dst[k] = src[k - qz];
    const int64_t head_end = min(qa << 2, gw1), tail_begin = max(qb << 2, head_end);
    if (gw0 + threadIdx.x < head_end) out[gw0 + threadIdx.x] = o32[pad + threadIdx.x];
    if (tail_begin + threadIdx.x < gw1) out[tail_begin + threadIdx.x] = o32[pad + (int)(tail_begin - gw0) + threadIdx.x];
}

// gsx_spz_layout -> SpzLayoutDev: the row size in range, every present field inside a row, bit f of `required` = field f must be
// present.  The format's own rules follow at the caller.
static int layout_to_dev(const gsx_spz_layout *l, uint64_t required, SpzLayoutDev *out, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (l->row_bytes < 1 || l->row_bytes > SPZ_MAX_ROW_BYTES)
        GSX_FAIL("%s: rows of %lld bytes (1 ... %d are supported)", who, (long long)l->row_bytes, SPZ_MAX_ROW_BYTES);
    out->row_bytes = (int)l->row_bytes;
    for (int f = 0; f < SPZ_FIELDS; ++f) {
        const int o = l->offset[f];
        if (o < 0) {
            if ((required >> f) & 1) GSX_FAIL("%s: field %d is required", who, f);
        } else if (o + 4 > l->row_bytes) {
            GSX_FAIL("%s: field %d at byte offset %d of a %lld-byte row", who, f, o, (long long)l->row_bytes);
        }
        out->off[f] = o < 0 ? -1 : o;
    }
    return 0;
}

// the ResidentRows contract of a table in HBM (`what`: how the refusal calls it): rows of 1 ... 512 bytes, a 16-byte aligned
// base, row 0 at byte 0 ... 15
static int rows_args(const void *rows_dev, int64_t first_byte, int64_t stride, const char *who, const char *what = "rows")
{
    if (stride < 1 || stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("%s: %s of %lld bytes (1 ... %d are supported)", who, what, (long long)stride, SPZ_MAX_ROW_BYTES);
    if (reinterpret_cast<uintptr_t>(rows_dev) & 15) GSX_FAIL("%s: %s must be 16-byte aligned", who, what);
    if (first_byte < 0 || first_byte > 15) GSX_FAIL("%s: the first row of the %s at byte %lld (0 ... 15)", who, what, (long long)first_byte);
    return 0;
}

// fields [0, f)
constexpr uint64_t fields_below(int f) { return (1ull << f) - 1; }

// grid size of a grid-stride kernel: one block per `per_block` items, at most `per_cu` blocks per compute unit, at least one
static unsigned tile_blocks(gsx_ctx *c, int64_t items, int per_block, int per_cu)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, (int64_t)c->num_cu * per_cu));
}

// a scan kernel's one 64-bit result word -> *mask_out: the context's nzmask word zeroed, launch(d_mask) on the context's stream,
// the word copied out, the stream joined
template <class Launch>
static int nzmask_word(gsx_ctx *c, uint64_t *mask_out, Launch launch)
{
    GSX_CHECK(c->nzmask.reserve(16));
    unsigned long long *d_mask = c->nzmask.as<unsigned long long>();
    GSX_HIP(hipMemsetAsync(d_mask, 0, 8, c->stream));
    launch(d_mask);
    GSX_HIP(hipGetLastError());
    GSX_HIP(hipMemcpyAsync(mask_out, d_mask, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- what the PLY reader's and the PLY writer's transcodes share (csrc/ply_read.hip, csrc/ply_write.hip): a workgroup of
// PLY_THREADS lanes per tile, the staged input and an image of the output tile both in LDS, a descriptor word per field / run

constexpr int PLY_NO_SRC = 0x3ff;             // descriptor: no source, the bytes stay zero
constexpr size_t PLY_MAX_LDS = 2 * 32768 + 256;
constexpr int PLY_THREADS = 256;              // lanes per workgroup: four waves share a tile of 128 or 64 rows

static int ply_strides(int in_stride, int out_stride, const char *who)
{
    if (in_stride < 1 || in_stride > SPZ_MAX_ROW_BYTES || out_stride < 1 || out_stride > SPZ_MAX_ROW_BYTES)
        GSX_FAIL("%s: row strides in %d, out %d (1 ... %d are supported)", who, in_stride, out_stride, SPZ_MAX_ROW_BYTES);
    return 0;
}

// output bytes [dof, dof + nb) are those of `noun` k ("field" / "run"): none of them may be another's
static int ply_cover(unsigned char *covered, int dof, int nb, const char *noun, int k, const char *who)
{
    for (int i = 0; i < nb; ++i) {
        if (covered[dof + i]) GSX_FAIL("%s: %s %d overlaps another at output byte %d", who, noun, k, dof + i);
        covered[dof + i] = 1;
    }
    return 0;
}

// every output byte written exactly once (nothing of the LDS image leaves unwritten), the descriptors from `used` on zeroed, the
// strides taken over; in_quads and tile_rows are ply_launch's
template <class Args, int N>
static int ply_args_finish(const unsigned char *covered, const char *noun, unsigned (&desc)[N], int used, int in_stride, int out_stride,
                           Args *A, const char *who)
{
    for (int i = 0; i < out_stride; ++i)
        if (!covered[i]) GSX_FAIL("%s: output byte %d belongs to no %s", who, i, noun);
    for (int k = used; k < N; ++k) desc[k] = 0u;
    A->in_stride = in_stride;
    A->out_stride = out_stride;
    A->in_quads = A->tile_rows = 0;
    return 0;
}

// n >= 1 rows through `kernel`, one workgroup per tile: the pointers checked (`in_name`: what the input is called), the tile of
// the larger stride, its LDS (A.in_quads and A.tile_rows are set here), launch(tiles, lds_bytes)
template <class Args, class Launch>
static int ply_launch(gsx_ctx *c, const void *kernel, Args &A, int64_t n, const void *in_dev, const char *in_name, const void *out_dev,
                      const char *who, Launch launch)
{
    if (!in_dev || !out_dev) GSX_FAIL("%s: null argument", who);
    if ((reinterpret_cast<uintptr_t>(in_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        GSX_FAIL("%s: %s and output must be 16-byte aligned", who, in_name);
    const int tr = spz_tile_rows(std::max(A.in_stride, A.out_stride));
    const int64_t tiles = (n + tr - 1) / tr;
    if (tiles >= (1LL << 31)) GSX_FAIL("%s: too many rows", who);
    const size_t in_bytes = spz_in_bytes(tr, A.in_stride);
    const size_t lds = in_bytes + ((size_t)tr * A.out_stride + 32 + 15) / 16 * 16;   // + what store_bytes reads behind the image
    A.in_quads = (int)(in_bytes / 16);
    A.tile_rows = tr;
    if (lds > PLY_MAX_LDS) GSX_FAIL("%s: a tile of %zu LDS bytes", who, lds);
    GSX_HIP(hipSetDevice(c->device));
    if (lds > 65536)   // two staged tiles of up to 32 KiB each: past the default limit of dynamic LDS, within the 160 KiB of a CU
        GSX_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PLY_MAX_LDS));
    launch((unsigned)tiles, lds);
    GSX_HIP(hipGetLastError());
    return 0;
}

}  // namespace gsx
