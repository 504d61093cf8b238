// transform.hip -- a similarity transform p' = s R p + t of a whole splat table, on the rows where they lie:
//
//   gsx_rows_transform_dev    resident rows (csrc/resident_rows.hip's addressing), in place or into a second buffer
//   gsx_rows_transform_host   the same per-row functions on a host table: the twin the host tests hold against the definition
//
// Four parts of a row depend on the frame: the position, the log-scales, the orientation quaternion and every spherical-harmonic
// band above DC (normals too, where a table has them).  The definition is tests/transform_numpy.py: every product and sum in
// float64, rounded once per operation and evaluated left to right (the build's -ffp-contract=off: no fma is written here), the
// result cast to float32; the log-scales take one float32 add.  Everything else in a row is a bit copy.
//
// A workgroup owns a tile of spz_tile_rows(stride) rows: the tile is staged in LDS (spz_stage_tile), the fields are rewritten in
// that image, and the image leaves through store_staged -- whole 16-byte quads where the tile covers them, its ragged ends byte by
// byte, so no two workgroups write the same byte and a tile's source bytes are all read before any of its bytes are written
// (out_dev may be rows_dev).  The work of a tile is cut into (task, row) items, task-major: a task is one part of a row with its
// own fields -- the position, the normals, the scales, the quaternion, one (channel, band) of the f_rest block -- so the 64 lanes
// of a wave run the same task on consecutive rows, and a lane loads its task's 3 ... 7 inputs before it stores the first output.
// The 83 matrix entries, M, R, t, q_R and the log of the scale are wave-uniform: they are copied from HBM into LDS once per tile.
#include <algorithm>

#include "row_tile.h"

namespace gsx {

enum { TF_POSITION = 0, TF_NORMALS, TF_SCALES, TF_QUAT, TF_BAND1, TF_BAND2, TF_BAND3 };
constexpr int TF_MAX_TASKS = 13;         // position, normals, scales, quaternion, 3 channels x 3 bands
constexpr int TF_THREADS = 256;

struct TfDev {
    double M[9], R[9], t[3], q[4], D1[9], D2[25], D3[49];
    float ls;
    int ntask;
    int kind[TF_MAX_TASKS + 1];
    int off[TF_MAX_TASKS + 1][7];          // byte offsets of the task's fields inside a row
};

// the float32 fields of a staged tile in LDS, at any byte
struct LdsMem {
    unsigned *w;
    __device__ __forceinline__ float ld(int q) const { return lds_f32(w, q); }
    __device__ __forceinline__ void st(int q, float v) const
    {
        const unsigned b = __float_as_uint(v);
        if ((q & 3) == 0) {
            w[q >> 2] = b;
        } else {                            // byte stores: a neighbouring field may share both words
            unsigned char *p = reinterpret_cast<unsigned char *>(w) + q;
            p[0] = (unsigned char)b;
            p[1] = (unsigned char)(b >> 8);
            p[2] = (unsigned char)(b >> 16);
            p[3] = (unsigned char)(b >> 24);
        }
    }
};

// ... of one host row
struct HostMem {
    unsigned char *p;
    float ld(int q) const
    {
        float v;
        memcpy(&v, p + q, 4);
        return v;
    }
    void st(int q, float v) const { memcpy(p + q, &v, 4); }
};

// out_i = f32(((A[i][0] X + A[i][1] Y) + A[i][2] Z) [+ t_i])
template <class Mem>
__host__ __device__ __forceinline__ void tf_affine(const Mem &m, int q, const int *off, const double *A, const double *t)
{
    const double X = (double)m.ld(q + off[0]), Y = (double)m.ld(q + off[1]), Z = (double)m.ld(q + off[2]);
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double acc = (A[3 * i] * X + A[3 * i + 1] * Y) + A[3 * i + 2] * Z;
        if (t) acc = acc + t[i];
        o[i] = (float)acc;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) m.st(q + off[i], o[i]);
}

template <class Mem>
__host__ __device__ __forceinline__ void tf_scales(const Mem &m, int q, const int *off, float ls)
{
    float o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = m.ld(q + off[i]) + ls;
#pragma unroll
    for (int i = 0; i < 3; ++i) m.st(q + off[i], o[i]);
}

// the Hamilton product q_R (x) q, q = rot_0..3; the norm is kept
template <class Mem>
__host__ __device__ __forceinline__ void tf_quat(const Mem &m, int q, const int *off, const double *qr)
{
    const double a = (double)m.ld(q + off[0]), b = (double)m.ld(q + off[1]), c = (double)m.ld(q + off[2]), d = (double)m.ld(q + off[3]);
    const double w = qr[0], x = qr[1], y = qr[2], z = qr[3];
    const float o0 = (float)(((w * a - x * b) - y * c) - z * d);
    const float o1 = (float)(((w * b + x * a) + y * d) - z * c);
    const float o2 = (float)(((w * c - x * d) + y * a) + z * b);
    const float o3 = (float)(((w * d + x * c) - y * b) + z * a);
    m.st(q + off[0], o0);
    m.st(q + off[1], o1);
    m.st(q + off[2], o2);
    m.st(q + off[3], o3);
}

// one band of one channel: out_j = f32((...((D[j][0] v_0 + D[j][1] v_1) + D[j][2] v_2) + ...))
template <int NB, class Mem>
__host__ __device__ __forceinline__ void tf_band(const Mem &m, int q, const int *off, const double *D)
{
    double v[NB];
    float o[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = (double)m.ld(q + off[k]);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        double acc = D[j * NB] * v[0];
#pragma unroll
        for (int k = 1; k < NB; ++k) acc = acc + D[j * NB + k] * v[k];
        o[j] = (float)acc;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) m.st(q + off[j], o[j]);
}

// task `task` of the row at byte q
template <class Mem>
__host__ __device__ __forceinline__ void tf_apply(const Mem &m, int q, const TfDev &P, int task)
{
    const int *off = P.off[task];
    switch (P.kind[task]) {
    case TF_POSITION: tf_affine(m, q, off, P.M, P.t); break;
    case TF_NORMALS: tf_affine(m, q, off, P.R, (const double *)nullptr); break;
    case TF_SCALES: tf_scales(m, q, off, P.ls); break;
    case TF_QUAT: tf_quat(m, q, off, P.q); break;
    case TF_BAND1: tf_band<3>(m, q, off, P.D1); break;
    case TF_BAND2: tf_band<5>(m, q, off, P.D2); break;
    default: tf_band<7>(m, q, off, P.D3); break;
    }
}

// spz_stage_tile's mirror: the staged image `lds` (LDS quad k holds the quad at byte 16 ((b0 >> 4) + k)) -> bytes [b0, b1) of
// `out` (16-byte aligned), by the whole workgroup: the quads the span covers whole as 16-byte stores, its ragged ends by bytes
__device__ __forceinline__ void store_staged(unsigned char *__restrict__ out, int64_t b0, int64_t b1, const uint4 *lds)
{
    const int64_t q0 = b0 >> 4, qa = (b0 + 15) >> 4, qb = b1 >> 4;
    const int64_t head_end = min(b1, qa << 4), tail_begin = max(head_end, qb << 4);
    const unsigned char *img = reinterpret_cast<const unsigned char *>(lds);   // img[b - 16 q0]: byte b of the table
    const int t = threadIdx.x;
    if (b0 + t < head_end) out[b0 + t] = img[(int)(b0 - (q0 << 4)) + t];
    if (tail_begin + t < b1) out[tail_begin + t] = img[(int)(tail_begin - (q0 << 4)) + t];
    uint4 *dst = reinterpret_cast<uint4 *>(out);
    for (int64_t k = qa + t; k < qb; k += blockDim.x) dst[k] = lds[k - q0];
}

__global__ __launch_bounds__(TF_THREADS, 4) void rows_transform_kernel(const uint4 *rows, int rb, int tr, int64_t first, int64_t n,
                                                                    const unsigned *__restrict__ plan, unsigned char *out)
{
    extern __shared__ uint4 tf_lds[];
    __shared__ TfDev s_P;
    for (int k = threadIdx.x; k < (int)(sizeof(TfDev) / 4); k += TF_THREADS) reinterpret_cast<unsigned *>(&s_P)[k] = plan[k];
    const int64_t t0 = (int64_t)blockIdx.x * tr;
    const int cnt = (int)min((int64_t)tr, n - t0);
    const int base = spz_stage_tile(rows, rb, t0, cnt, tf_lds, first);
    __syncthreads();
    const LdsMem mem = {reinterpret_cast<unsigned *>(tf_lds)};
    // tr lanes (one or two waves) per task, TF_THREADS / tr tasks at a time: the task is the same for a whole wave
    const int r = (int)threadIdx.x % tr, ntask = s_P.ntask;
    for (int task = __builtin_amdgcn_readfirstlane((int)threadIdx.x / tr); task < ntask; task += TF_THREADS / tr) {
        __asm__ volatile("" ::: "memory");   // a task's matrix is read where it is used: all 108 entries held at once spill
        if (r < cnt) tf_apply(mem, base + r * rb, s_P, task);
    }
    __syncthreads();
    const int64_t b0 = first + t0 * rb;
    store_staged(out, b0, b0 + (int64_t)cnt * rb, tf_lds);
}

// gsx_transform_layout -> the task list: every field of an active part inside a row, no byte written by two tasks
static int tf_plan(const gsx_transform_layout *l, int64_t stride, TfDev *P, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (stride < 1 || stride > SPZ_MAX_ROW_BYTES) GSX_FAIL("%s: rows of %lld bytes (1 ... %d are supported)", who, (long long)stride, SPZ_MAX_ROW_BYTES);
    if (l->parts & ~(uint32_t)GSX_TF_ALL) GSX_FAIL("%s: parts 0x%x", who, l->parts);
    memset(P, 0, sizeof(*P));
    memcpy(P->M, l->M, sizeof(P->M));
    memcpy(P->R, l->R, sizeof(P->R));
    memcpy(P->t, l->t, sizeof(P->t));
    memcpy(P->q, l->q, sizeof(P->q));
    memcpy(P->D1, l->D1, sizeof(P->D1));
    memcpy(P->D2, l->D2, sizeof(P->D2));
    memcpy(P->D3, l->D3, sizeof(P->D3));
    P->ls = l->log_scale;
    unsigned char covered[SPZ_MAX_ROW_BYTES];
    memset(covered, 0, sizeof(covered));
    auto add = [&](int kind, const int32_t *off, int count, const char *what) -> int {
        int *dst = P->off[P->ntask];
        for (int k = 0; k < count; ++k) {
            const int o = off[k];
            if (o < 0 || o + 4 > stride) GSX_FAIL("%s: %s field %d at byte offset %d of a %lld-byte row", who, what, k, o, (long long)stride);
            for (int b = o; b < o + 4; ++b) {
                if (covered[b]) GSX_FAIL("%s: %s field %d overlaps another written field at byte %d", who, what, k, b);
                covered[b] = 1;
            }
            dst[k] = o;
        }
        P->kind[P->ntask++] = kind;
        return 0;
    };
    if (l->parts & GSX_TF_POSITION) GSX_CHECK(add(TF_POSITION, l->xyz_offset, 3, "position"));
    if (l->parts & GSX_TF_NORMALS) GSX_CHECK(add(TF_NORMALS, l->normal_offset, 3, "normal"));
    if (l->parts & GSX_TF_SCALES) GSX_CHECK(add(TF_SCALES, l->scale_offset, 3, "scale"));
    if (l->parts & GSX_TF_ROTATION) GSX_CHECK(add(TF_QUAT, l->rot_offset, 4, "rotation"));
    const int m = l->rest_m;
    for (int band = 3; band >= 1; --band) {     // (the widest band first: its items are the longest)
        if (!(l->parts & (GSX_TF_SH1 << (band - 1)))) continue;
        if (m < band * band + 2 * band || m > 15) GSX_FAIL("%s: SH band %d of %d coefficients per channel", who, band, m);
        for (int c = 0; c < 3; ++c) GSX_CHECK(add(TF_BAND1 + band - 1, l->rest_offset + c * m + band * band - 1, 2 * band + 1, "f_rest"));
    }
    return 0;
}

}  // namespace gsx

using namespace gsx;

extern "C" int gsx_rows_transform_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n,
                                      const gsx_transform_layout *layout, void *out_dev)
{
    if (!c || (n > 0 && (!rows_dev || !out_dev))) GSX_FAIL("gsx_rows_transform_dev: null argument");
    if (n < 0 || n >= (1LL << 32)) GSX_FAIL("gsx_rows_transform_dev: %lld rows", (long long)n);
    TfDev P;
    GSX_CHECK(tf_plan(layout, stride, &P, "gsx_rows_transform_dev"));
    if ((reinterpret_cast<uintptr_t>(rows_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        GSX_FAIL("gsx_rows_transform_dev: rows and output must be 16-byte aligned");
    if (first_byte < 0 || first_byte > 15) GSX_FAIL("gsx_rows_transform_dev: the first row at byte %lld (0 ... 15)", (long long)first_byte);
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    const int rb = (int)stride, tr = spz_tile_rows(rb);
    const int64_t tiles = (n + tr - 1) / tr;
    GSX_CHECK(c->work.reserve(sizeof(TfDev)));
    GSX_HIP(hipMemcpyAsync(c->work.p, &P, sizeof(TfDev), hipMemcpyHostToDevice, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));   // (P is this frame's)
    hipLaunchKernelGGL(rows_transform_kernel, dim3((unsigned)tiles), dim3(TF_THREADS), spz_in_bytes(tr, rb), c->stream,
                       static_cast<const uint4 *>(rows_dev), rb, tr, first_byte, n, c->work.as<unsigned>(), static_cast<unsigned char *>(out_dev));
    GSX_HIP(hipGetLastError());
    return 0;
}

extern "C" int gsx_rows_transform_host(const void *rows, int64_t stride, int64_t n, const gsx_transform_layout *layout, void *out)
{
    if (n > 0 && (!rows || !out)) GSX_FAIL("gsx_rows_transform_host: null argument");
    if (n < 0) GSX_FAIL("gsx_rows_transform_host: %lld rows", (long long)n);
    TfDev P;
    GSX_CHECK(tf_plan(layout, stride, &P, "gsx_rows_transform_host"));
    const unsigned char *src = static_cast<const unsigned char *>(rows);
    unsigned char *dst = static_cast<unsigned char *>(out);
    for (int64_t r = 0; r < n; ++r) {
        unsigned char *row = dst + r * stride;
        if (row != src + r * stride) memcpy(row, src + r * stride, (size_t)stride);
        const HostMem mem = {row};
        for (int task = 0; task < P.ntask; ++task) tf_apply(mem, 0, P, task);
    }
    return 0;
}
