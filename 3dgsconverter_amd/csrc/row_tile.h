// row_tile.h -- the row-tile staging shared by the writers that read a raw splat table in place (csrc/spz.hip, csrc/ksplat.hip).
//
// A workgroup owns a tile of consecutive rows: the tile's raw bytes are staged in LDS with 16-byte loads (any row size up to
// 512 bytes, fields at any byte offset: a field is assembled from two LDS words).  The layout is gsx_spz_layout's: float32
// fields in gsx_sog_layout's order, -1 = absent.
#pragma once
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

// the tile's rows [t0, t0 + cnt) -> LDS, from the 16-byte boundary at or below the first byte; -> that boundary's offset.
// Reads at most 15 bytes past the last row (the caller's allocation has that slack).
__device__ __forceinline__ int spz_stage_tile(const uint4 *__restrict__ rows, int row_bytes, int64_t t0, int cnt, uint4 *lds)
{
    const int64_t b0 = t0 * row_bytes, b1 = (t0 + cnt) * row_bytes;
    const int64_t q0 = b0 >> 4, q1 = (b1 + 15) >> 4;
    const int nq = (int)(q1 - q0);
    for (int k = threadIdx.x; k < nq; k += blockDim.x) lds[k] = rows[q0 + k];
    return (int)(b0 & 15);
}

// the float32 at LDS byte index q (any alignment)
__device__ __forceinline__ float spz_lds_f32(const unsigned *lds, int q)
{
    const unsigned lo = lds[q >> 2], hi = lds[(q >> 2) + 1];
    return __uint_as_float(__builtin_amdgcn_alignbyte(hi, lo, (unsigned)(q & 3)));
}

// np.clip(t, 0, 255).astype(np.uint8): NaN stays NaN through the clip and casts to 0
__device__ __forceinline__ unsigned spz_u8(float t)
{
    return t == t ? (unsigned)fminf(fmaxf(t, 0.0f), 255.0f) : 0u;
}

}  // namespace gsx
