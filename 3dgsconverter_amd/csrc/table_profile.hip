// table_profile.hip -- gsx_table_profile_dev: the SH-activity word, the coordinate bounds and the NaN flags of a resident table
// in one pass over its rows.
//
//   converter.py:121-146     the source SH degree: np.any(self.data[f'f_rest_{i}'] != 0), one strided column at a time
//   main.py:109-114,190-209  the info block: six strided min / max reductions, up to 45 more np.any scans
//
// The readers hold the decoded rows in HBM just before their download; the pass there reads the table once and writes 40 bytes.
// The tile staging is row_tile.h's, the bit test rest_scan.h's, the float order sog_math.h's sort_key.  Every accumulator is an
// OR or a maximum of unsigned words that starts from zero (the minimum is kept as the maximum of the inverted key), so the
// result does not depend on the order the workgroups arrive in.  The host twin is csrc/host_rows.hip's gsx_table_profile_host.
#include "row_tile.h"
#include "sog_math.h"
#include "table_profile.h"

namespace gsx {

struct ProfileAcc {                      // zeroed before the launch
    unsigned long long rest;
    unsigned nlo[3];                     // max of ~sort_key(v) over the non-NaN v: 0 = none seen
    unsigned hi[3];                      // max of sort_key(v): 0 = none seen (no float has the key 0)
    unsigned nan;
    unsigned pad;
};

__device__ __forceinline__ unsigned wave_max(unsigned v)
{
    for (int m = WAVE / 2; m; m >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, m, WAVE));
    return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v)
{
    for (int m = WAVE / 2; m; m >>= 1) v |= (unsigned)__shfl_xor((int)v, m, WAVE);
    return v;
}

// one lane per row of a staged tile; blockDim.x = spz_tile_rows(rb), a multiple of the wave.  ALIGNED: the row size, the first
// byte and every offset are multiples of 4 (the canonical tables), so a field is one LDS word and not two
template <bool ALIGNED>
__global__ void table_profile_kernel(const uint4 *__restrict__ rows, int rb, int64_t first, int64_t n, ProfileOffsets O,
                                     unsigned long long present, ProfileAcc *__restrict__ acc)
{
    extern __shared__ uint4 tp_lds[];
    __shared__ ProfileAcc s_acc;
    __shared__ int off[PROFILE_FIELDS];                           // (dynamic indices: LDS, not SGPRs)
    if ((int)threadIdx.x < PROFILE_FIELDS) off[threadIdx.x] = O.off[threadIdx.x];
    if (threadIdx.x == 0) {
        s_acc.rest = 0ull;
        for (int a = 0; a < 3; ++a) s_acc.nlo[a] = s_acc.hi[a] = 0u;
        s_acc.nan = 0u;
    }
    const int tr = blockDim.x;
    const unsigned *in32 = reinterpret_cast<const unsigned *>(tp_lds);
    unsigned long long bits = 0ull;
    unsigned nlo[3] = {0u, 0u, 0u}, hi[3] = {0u, 0u, 0u}, nan = 0u;
    const int64_t ntiles = (n + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * tr;
        const int cnt = (int)min((int64_t)tr, n - t0);
        __syncthreads();
        const int base = spz_stage_tile(rows, rb, t0, cnt, tp_lds, first);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int q = base + (int)threadIdx.x * rb;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if ((present >> a) & 1ull) {
                    const float v = ALIGNED ? __uint_as_float(in32[(q + off[a]) >> 2]) : lds_f32(in32, q + off[a]);
                    if (v != v) {
                        nan |= 1u << a;
                    } else {
                        const unsigned k = sort_key(v);
                        nlo[a] = max(nlo[a], ~k);
                        hi[a] = max(hi[a], k);
                    }
                }
            for (int i = 0; i < 45; ++i)
                if ((present >> (3 + i)) & 1ull) {
                    const unsigned w = ALIGNED ? in32[(q + off[3 + i]) >> 2] : lds_u32(in32, q + off[3 + i]);
                    bits |= (unsigned long long)((w & 0x7fffffffu) != 0u) << i;
                }
        }
    }
    // wave reduction, then one LDS combine per wave
    const unsigned blo = wave_or((unsigned)bits), bhi = wave_or((unsigned)(bits >> 32));
    for (int a = 0; a < 3; ++a) {
        nlo[a] = wave_max(nlo[a]);
        hi[a] = wave_max(hi[a]);
    }
    nan = wave_or(nan);
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        atomicOr(&s_acc.rest, ((unsigned long long)bhi << 32) | blo);
        for (int a = 0; a < 3; ++a) {
            atomicMax(&s_acc.nlo[a], nlo[a]);
            atomicMax(&s_acc.hi[a], hi[a]);
        }
        atomicOr(&s_acc.nan, nan);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_acc.rest) atomicOr(&acc->rest, s_acc.rest);
        for (int a = 0; a < 3; ++a) {
            if (s_acc.nlo[a]) atomicMax(&acc->nlo[a], s_acc.nlo[a]);
            if (s_acc.hi[a]) atomicMax(&acc->hi[a], s_acc.hi[a]);
        }
        if (s_acc.nan) atomicOr(&acc->nan, s_acc.nan);
    }
}

}  // namespace gsx

using namespace gsx;

extern "C" int gsx_table_profile_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t n, const gsx_profile_layout *layout,
                                     gsx_table_profile *out)
{
    if (!c || !rows_dev || !out) GSX_FAIL("gsx_table_profile_dev: null argument");
    ProfileOffsets O;
    GSX_CHECK(profile_layout_check(layout, n, &O, "gsx_table_profile_dev"));
    if (reinterpret_cast<uintptr_t>(rows_dev) & 15) GSX_FAIL("gsx_table_profile_dev: rows must be 16-byte aligned");
    if (first_byte < 0 || first_byte > 15) GSX_FAIL("gsx_table_profile_dev: the first row at byte %lld (0 ... 15)", (long long)first_byte);
    unsigned long long present = 0ull;
    const int rb = (int)layout->row_bytes;
    bool aligned = !(rb & 3) && !(first_byte & 3);
    for (int f = 0; f < PROFILE_FIELDS; ++f)
        if (O.off[f] >= 0) {
            present |= 1ull << f;
            aligned = aligned && !(O.off[f] & 3);
        } else {
            O.off[f] = 0;                                         // never read
        }
    const int tr = spz_tile_rows(rb);
    GSX_HIP(hipSetDevice(c->device));
    GSX_CHECK(c->nzmask.reserve(sizeof(ProfileAcc)));
    ProfileAcc *d_acc = c->nzmask.as<ProfileAcc>();
    GSX_HIP(hipMemsetAsync(d_acc, 0, sizeof(ProfileAcc), c->stream));
    hipLaunchKernelGGL(aligned ? table_profile_kernel<true> : table_profile_kernel<false>, dim3(tile_blocks(c, n, tr, 8)), dim3(tr), spz_in_bytes(tr, rb), c->stream,
                       static_cast<const uint4 *>(rows_dev), rb, first_byte, n, O, present, d_acc);
    GSX_HIP(hipGetLastError());
    ProfileAcc h;
    GSX_HIP(hipMemcpyAsync(&h, d_acc, sizeof(ProfileAcc), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    out->rest_nonzero = h.rest;
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = h.nlo[a] ? sort_unkey(~h.nlo[a]) : __builtin_inff();
        out->hi[a] = h.hi[a] ? sort_unkey(h.hi[a]) : -__builtin_inff();
    }
    out->nan_axes = h.nan;
    out->n = n;
    return 0;
}
