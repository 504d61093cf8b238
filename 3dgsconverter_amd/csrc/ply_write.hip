// ply_write.hip -- the 3DGS / CloudCompare PLY writers' row pack: the rows of a structured table as the caller holds them -> the
// rows of the file's vertex element, byte for byte; and the scan behind `crop_sh`.
//
// Replaces, in gsconverter/formats/ply_3dgs.py (Ply3DGSFormat.write) and gsconverter/formats/ply_cc.py (PlyCCFormat.write):
//   the crop scan           ply_3dgs.py:70-76   ply_cc.py:70-76    `np.any(data[f_rest_i] != 0)` from i = 44 down, up to 45 strided
//                                                                  scans -> one pass over the resident rows for every field at once
//   the zeroed table        ply_3dgs.py:104     ply_cc.py:112      a run without a source writes zero
//   the copy loop           ply_3dgs.py:107-109 ply_cc.py:115-116  `output_data[name] = data[name]`, up to 65 strided column copies
//                                                                  -> one pass over the rows, driven by a run table
// Which fields the file holds, their order and their names (has_rgb, crop_sh, the padded normals and f_rest, the extras, the
// scalar_ prefix of the CloudCompare writer) are the host's business (formats/ply_writer.py: plan_write); the two writers share
// these kernels.  Nothing is cast: a field keeps the table's type, so every field is a byte copy, and fields that follow each
// other in the table and in the file are one copy.  The host merges them into RUNS (source byte offset or none = zero fill,
// destination byte offset, bytes): 1 ... 5 runs a row on the canonical tables, not 62 fields.
//
// A workgroup of 256 lanes owns a tile of consecutive rows (spz_tile_rows on the larger stride: 128 rows, or 64 when a stride is
// over 256 bytes): the tile's raw bytes are staged in LDS with 16-byte loads from any starting byte, the runs are moved into an
// LDS image of the output tile, and the image leaves in 16-byte stores (row_tile.h).  A run is walked run by run (uniform: its
// descriptor is a scalar load from the kernel arguments) with consecutive lanes on consecutive dwords of a row -- consecutive
// LDS banks on both sides.  The destination decides the shape of a copy: the bytes up to its first 4-byte boundary and behind
// its last one are byte stores by one lane, every dword between them is one ds_write_b32 whose value is assembled from the two
// source words around it (lds_u32), so the source may sit at any byte: rows of 251 bytes change their alignment from row to row
// and still move as dwords.
#include "gsx_common.h"
#include "row_tile.h"
#include "rest_scan.h"

namespace gsx {

constexpr int PLYW_MAX_RUNS = GSX_PLY_WRITE_MAX_RUNS;

struct PlyWriteArgs {
    int in_stride, out_stride, n_runs, in_quads, tile_rows;
    unsigned run[PLYW_MAX_RUNS];              // src offset (10 bits, PLY_NO_SRC = none) | dst offset << 10 | (bytes - 1) << 20
};

// the units of a run of nb bytes: unit 0 = the bytes outside the destination's aligned dwords, units 1 ... nb / 4 = those dwords
// (a destination that starts off a boundary has one dword fewer: its last unit does nothing)
__host__ __device__ inline int ply_run_units(int nb) { return 1 + (nb >> 2); }

// unit u of one run of one row: nb bytes from byte s0 of the source (fill: zeros instead) to byte d0 of the destination, whose
// alignment is d0's.  src.byte(q) / src.word(q): the byte / little-endian u32 at source byte q (any q); dst.byte(o, v): one
// byte; dst.word(o, v): the u32 at destination byte o, o a multiple of 4
template <class Src, class Dst>
__host__ __device__ inline void ply_run_unit(const Src &src, const Dst &dst, bool fill, int s0, int d0, int nb, int u)
{
    const int lead = (4 - (d0 & 3)) & 3;
    const int head = lead < nb ? lead : nb;
    const int body = (nb - head) >> 2;
    if (u == 0) {
        for (int i = 0; i < head; ++i) dst.byte(d0 + i, fill ? 0u : src.byte(s0 + i));
        for (int i = head + 4 * body; i < nb; ++i) dst.byte(d0 + i, fill ? 0u : src.byte(s0 + i));
    } else if (u <= body) {
        const int o = head + 4 * (u - 1);
        dst.word(d0 + o, fill ? 0u : src.word(s0 + o));
    }
}

struct PlyLdsSrc {
    const unsigned *lds;
    __device__ __forceinline__ unsigned byte(int q) const { return lds_u8(lds, q); }
    __device__ __forceinline__ unsigned word(int q) const { return lds_u32(lds, q); }
};

struct PlyLdsDst {
    unsigned char *img;
    __device__ __forceinline__ void byte(int o, unsigned v) const { img[o] = (unsigned char)v; }
    __device__ __forceinline__ void word(int o, unsigned v) const { *reinterpret_cast<unsigned *>(img + o) = v; }
};

// one workgroup of PLY_THREADS lanes per tile of A.tile_rows rows; rows [0, n)
__global__ __launch_bounds__(PLY_THREADS) void ply_pack_kernel(const uint4 *__restrict__ rows, int64_t n, PlyWriteArgs A, unsigned char *__restrict__ out)
{
    extern __shared__ uint4 pw_lds[];
    const int tr = A.tile_rows;
    const int64_t t0 = (int64_t)blockIdx.x * tr;
    if (t0 >= n) return;   // (uniform; the grid covers [0, n) exactly)
    const int cnt = (int)min((int64_t)tr, n - t0);
    const int base = spz_stage_tile(rows, A.in_stride, t0, cnt, pw_lds);
    const PlyLdsSrc src{reinterpret_cast<const unsigned *>(pw_lds)};
    unsigned char *img = reinterpret_cast<unsigned char *>(pw_lds + A.in_quads);
    const PlyLdsDst dst{img};
    __syncthreads();
    for (int k = 0; k < A.n_runs; ++k) {
        const unsigned d = A.run[k];
        const int so = (int)(d & 0x3ffu), dof = (int)((d >> 10) & 0x3ffu), nb = (int)(d >> 20) + 1;
        const bool fill = so == PLY_NO_SRC;
        const unsigned units = (unsigned)ply_run_units(nb), items = (unsigned)cnt * units;
        for (unsigned p = threadIdx.x; p < items; p += PLY_THREADS) {
            const unsigned r = p / units, u = p - r * units;
            ply_run_unit(src, dst, fill, base + (int)r * A.in_stride + so, (int)r * A.out_stride + dof, nb, (int)u);
        }
    }
    __syncthreads();
    const int64_t g0 = t0 * A.out_stride;
    store_bytes(out, g0, g0 + (int64_t)cnt * A.out_stride, img);
}

// gsx_ply_write_layout -> PlyWriteArgs: strides and counts in range, every source inside an input row, the runs tile the output
// row (every byte written exactly once: nothing of the LDS image leaves unwritten)
static int ply_write_layout_to_args(const gsx_ply_write_layout *l, PlyWriteArgs *A, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    GSX_CHECK(ply_strides(l->in_stride, l->out_stride, who));
    if (l->n_runs < 1 || l->n_runs > PLYW_MAX_RUNS) GSX_FAIL("%s: %d runs (1 ... %d are supported)", who, l->n_runs, PLYW_MAX_RUNS);
    unsigned char covered[SPZ_MAX_ROW_BYTES] = {0};
    for (int k = 0; k < l->n_runs; ++k) {
        const int so = l->src_offset[k], dof = l->dst_offset[k], nb = l->bytes[k];
        if (nb < 1 || dof < 0 || dof + nb > l->out_stride) GSX_FAIL("%s: run %d of %d bytes at byte offset %d of a %d-byte output row", who, k, nb, dof, l->out_stride);
        if (so < -1 || (so >= 0 && so + nb > l->in_stride)) GSX_FAIL("%s: run %d reads %d bytes at offset %d of a %d-byte row", who, k, nb, so, l->in_stride);
        GSX_CHECK(ply_cover(covered, dof, nb, "run", k, who));
        A->run[k] = (unsigned)(so < 0 ? PLY_NO_SRC : so) | ((unsigned)dof << 10) | ((unsigned)(nb - 1) << 20);
    }
    A->n_runs = l->n_runs;
    return ply_args_finish(covered, "run", A->run, l->n_runs, l->in_stride, l->out_stride, A, who);
}

struct PlyHostSrc {
    const unsigned char *rows;
    unsigned byte(int q) const { return rows[q]; }
    unsigned word(int q) const { return (unsigned)rows[q] | ((unsigned)rows[q + 1] << 8) | ((unsigned)rows[q + 2] << 16) | ((unsigned)rows[q + 3] << 24); }
};

struct PlyHostDst {
    unsigned char *img;
    void byte(int o, unsigned v) const { img[o] = (unsigned char)v; }
    void word(int o, unsigned v) const
    {
        img[o] = (unsigned char)v;
        img[o + 1] = (unsigned char)(v >> 8);
        img[o + 2] = (unsigned char)(v >> 16);
        img[o + 3] = (unsigned char)(v >> 24);
    }
};

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_ply_pack_dev(gsx_ctx *c, const void *rows_dev, int64_t n, const gsx_ply_write_layout *layout, void *out_dev)
{
    if (!c) GSX_FAIL("gsx_ply_pack_dev: null argument");
    PlyWriteArgs A;
    GSX_CHECK(ply_write_layout_to_args(layout, &A, "gsx_ply_pack_dev"));
    if (n < 0) GSX_FAIL("gsx_ply_pack_dev: n >= 0");
    if (n == 0) return 0;
    return ply_launch(c, reinterpret_cast<const void *>(ply_pack_kernel), A, n, rows_dev, "rows", out_dev, "gsx_ply_pack_dev",
                      [&](unsigned tiles, size_t lds) {
                          hipLaunchKernelGGL(ply_pack_kernel, dim3(tiles), dim3(PLY_THREADS), lds, c->stream, static_cast<const uint4 *>(rows_dev), n, A,
                                             static_cast<unsigned char *>(out_dev));
                      });
}

int gsx_ply_pack_host(const void *rows, int64_t n, const gsx_ply_write_layout *layout, void *out)
{
    PlyWriteArgs A;
    GSX_CHECK(ply_write_layout_to_args(layout, &A, "gsx_ply_pack_host"));
    if (n < 0 || (n > 0 && (!rows || !out))) GSX_FAIL("gsx_ply_pack_host: bad arguments");
    const int tr = spz_tile_rows(std::max(A.in_stride, A.out_stride));
    // tile by tile as the kernel walks them, so that a destination's alignment inside its tile image is the kernel's
    for (int64_t t0 = 0; t0 < n; t0 += tr) {
        const int cnt = (int)std::min<int64_t>(tr, n - t0);
        const PlyHostSrc src{static_cast<const unsigned char *>(rows) + t0 * A.in_stride};
        const PlyHostDst dst{static_cast<unsigned char *>(out) + t0 * A.out_stride};
        for (int k = 0; k < A.n_runs; ++k) {
            const unsigned d = A.run[k];
            const int so = (int)(d & 0x3ffu), dof = (int)((d >> 10) & 0x3ffu), nb = (int)(d >> 20) + 1;
            const int units = ply_run_units(nb);
            for (int p = 0; p < cnt * units; ++p)
                ply_run_unit(src, dst, so == PLY_NO_SRC, (p / units) * A.in_stride + so, (p / units) * A.out_stride + dof, nb, p % units);
        }
    }
    return 0;
}

int gsx_ply_rest_nonzero_dev(gsx_ctx *c, const void *rows_dev, int64_t stride, int64_t n, const int32_t *offsets, uint64_t present_mask,
                             uint64_t *mask_out)
{
    if (!c || !mask_out || !offsets || (n > 0 && !rows_dev)) GSX_FAIL("gsx_ply_rest_nonzero_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_ply_rest_nonzero_dev: 0 <= n < 2^32");
    if (present_mask >> 45) GSX_FAIL("gsx_ply_rest_nonzero_dev: fields beyond f_rest_44");
    if (stride < 1 || stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("gsx_ply_rest_nonzero_dev: rows of %lld bytes (1 ... %d are supported)", (long long)stride, SPZ_MAX_ROW_BYTES);
    if (reinterpret_cast<uintptr_t>(rows_dev) & 15) GSX_FAIL("gsx_ply_rest_nonzero_dev: rows must be 16-byte aligned");
    RestOffsets O;
    for (int i = 0; i < 45; ++i) {
        const bool on = (present_mask >> i) & 1;
        if (on && (offsets[i] < 0 || offsets[i] + 4 > stride)) GSX_FAIL("gsx_ply_rest_nonzero_dev: f_rest_%d at byte offset %d of a %lld-byte row", i, offsets[i], (long long)stride);
        O.off[i] = on ? offsets[i] : 0;
    }
    GSX_HIP(hipSetDevice(c->device));
    *mask_out = 0;
    if (n == 0 || present_mask == 0) return 0;
    return rest_scan(c, rows_dev, (int)stride, n, O, present_mask, mask_out);
}

}  // extern "C"
