// rest_scan.h -- the f_rest scan of the SPZ, .ksplat and PLY writers (csrc/spz.hip: gsx_spz_rest_nonzero_dev, csrc/ply_write.hip:
// gsx_ply_rest_nonzero_dev): `np.any(data[f_rest_i] != 0)` for up to 45 strided columns of a resident table in one pass over its
// rows (spz.py:60-77, ksplat.py:340-368, ply_3dgs.py:74, ply_cc.py:74).  The entry points check their own arguments and hand
// over 45 byte offsets; the tile staging is row_tile.h's.
#pragma once
#include "row_tile.h"

namespace gsx {

struct RestOffsets {
    int off[45];   // byte offset of f_rest_i inside a row (any value where bit i of `want` is clear: never read)
};

// bit i of *mask = some row holds f_rest_i != 0 (NaN and denormals count, -0.0 does not: the test is on the bits, whatever the
// denormal mode), for the fields in `want`.  static: both users compile their own copy
static __global__ void rest_scan_kernel(const uint4 *__restrict__ rows, int rb, int64_t n, RestOffsets O, unsigned long long want,
                                        unsigned long long *__restrict__ mask)
{
    extern __shared__ uint4 rs_lds[];
    __shared__ unsigned long long acc;
    __shared__ int off[45];                                       // (dynamic indices: LDS, not SGPRs)
    if ((int)threadIdx.x < 45) off[threadIdx.x] = O.off[threadIdx.x];
    const int tr = blockDim.x;
    const unsigned *in32 = reinterpret_cast<const unsigned *>(rs_lds);
    if (threadIdx.x == 0) acc = 0ull;
    unsigned long long bits = 0ull;
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();
        const int base = spz_stage_tile(rows, rb, t0, cnt, rs_lds);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int q = base + (int)threadIdx.x * rb;
            for (int i = 0; i < 45; ++i)
                if (((want >> i) & 1ull) && !((bits >> i) & 1ull) && (lds_u32(in32, q + off[i]) & 0x7fffffffu) != 0u) bits |= 1ull << i;
        }
    }
    __syncthreads();
    if (bits) atomicOr(&acc, bits);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicOr(mask, acc);
}

// n >= 1 rows of rb bytes (1 ... SPZ_MAX_ROW_BYTES, 16-byte aligned, 15 readable bytes behind the last row), want != 0 and every
// wanted offset inside a row: the caller has checked all of that -> *mask_out
static int rest_scan(gsx_ctx *c, const void *rows_dev, int rb, int64_t n, const RestOffsets &O, uint64_t want, uint64_t *mask_out)
{
    const int tr = spz_tile_rows(rb);
    return nzmask_word(c, mask_out, [&](unsigned long long *d_mask) {
        hipLaunchKernelGGL(rest_scan_kernel, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), spz_in_bytes(tr, rb), c->stream,
                           static_cast<const uint4 *>(rows_dev), rb, n, O, (unsigned long long)want, d_mask);
    });
}

}  // namespace gsx
