// decimate.hip -- voxel decimation (--decimate_voxel_size): all splats of a voxel become the one Gaussian that has their combined
// weight, mean and covariance.  No counterpart in the reference; the definition is tests/decimate_numpy.py, and
// every sum, product, division and root here is that file's, in its order: float64 rounded once per operation (the build's
// -ffp-contract=off: no fma is written here), division and root correctly rounded (__ddiv_rn, __dsqrt_rn, as the KNN epilogue and
// the compressed-PLY reader pin theirs), the float32 exp and log of np_exp.h / np_log.h.
//
//   gsx_rows_decimate_work_dev    bytes of workspace for n rows
//   gsx_rows_decimate_plan_dev    (a) keys  (b) stable order  (c) heads, sizes, slots, blocks; the one readback of the step
//   gsx_rows_decimate_write_dev   (d) block sums  (e) finish: partials of long groups, eigen-solve, output rows, single rows
//
// (a) one lane per listed row: the eleven geometry fields from the packed rows where they lie (any stride, any first byte), the
//     mergeable predicate, the visibility weight as float32, the 63-bit cell key (a row that is not mergeable: bit 63 | its place
//     in the list, a key of its own), and the refusal flag of a cell outside +-2^20.
// (b) rocprim's stable radix sort of (key, place): equal keys keep their row order, so a group's members follow one another in
//     row order and its first member is its lowest row.
// (c) run heads of the sorted keys -> group ids (an inclusive scan), head positions, sizes; the first member of every group is
//     flagged in row order and one exclusive scan gives its output slot: groups leave in the order of their first member.  A
//     third scan numbers the 256-member blocks of the groups of two rows or more.  No second sort, no atomics that order anything.
// (d) one wave per (group, block of <= 256 members).  64 members at a time: lane m computes member m's ten geometry terms
//     (W | S1 | S2) into LDS, then lane c walks the members in order and adds channel c -- its geometry term from LDS, or
//     w * field c of the member's row straight from HBM (consecutive lanes read consecutive words of a row).  A group of one
//     block is finished by the same wave; a longer group's block leaves its 64 float64 sums in HBM.
// (e) one wave per group above 256 rows adds its partials in block order and finishes: moments, six Jacobi sweeps, Shepperd,
//     the output row assembled in LDS over the first member's bytes and stored 16 bytes at a time.  Rows that are a group of
//     their own are copied by 16 lanes each.  Every kernel writes only the bytes of its own output rows.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "np_log.h"
#include "row_tile.h"

namespace gsx {

constexpr int DEC_BLOCK = 256;                   // members per block of a group's sums
constexpr int DEC_GEO = 10;                      // W | S1 x y z | S2 xx xy xz yy yz zz
constexpr int DEC_CELL_BIAS = 1 << 20;
constexpr int DEC_SLOT = 128;                    // a long group's block b keeps its partial sums at slot ceil(head / 128) + b
constexpr int DEC_ROW_QUADS = SPZ_MAX_ROW_BYTES / 16 + 2;   // LDS quads of one staged row (+ what lds_u32 reads behind it)
enum { DEC_ST_STATUS = 0, DEC_ST_MERGED, DEC_ST_LONG, DEC_ST_WORDS = 4 };

struct DecKeyArgs {
    int xyz[3], scale[3], rot[4], opacity;
    float h;                                     // (float)voxel_size
};

struct DecArgs {
    double H;
    int stride, n_mean, n_u8, n_zero;
    int xyz[3], scale[3], rot[4], opacity;
    short mean[GSX_DECIMATE_MAX_MEAN];
    short u8[3];
    short zero[GSX_DECIMATE_MAX_ZERO];
};

// the carve-up of the caller's workspace for n rows
struct DecWs {
    unsigned long long *keys0, *keys1;           // keys by place in the list | sorted.  keys0 is dead after the sort:
    unsigned *flag, *nblk_in;                    //   ... its bytes hold the scans' inputs (n | n + 1 words)
    unsigned *order;                             // sorted position -> place in the list
    float *w;                                    // by place: the weight
    unsigned *gincl;                             // by sorted position: group id (key order) + 1
    unsigned *heads;                             // group -> sorted position of its first member; heads[G] = n
    unsigned *fsz;                               // by place: rows of the group whose first member this is, else 0
    unsigned *slot;                              // by place: output row of a first member
    unsigned *item0;                             // group -> its first (group, block) item; item0[n] = all items
    unsigned *longs;                             // groups above 256 rows, in no particular order
    double *partial;                             // [n / 128 + 2][64]
    unsigned *state;
    void *temp;
    size_t temp_bytes, total;
};

static size_t dec_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int dec_carve(int64_t n, void *base, hipStream_t stream, DecWs *w)
{
    size_t t_sort = 0, t_incl = 0, t_excl = 0;
    unsigned long long *k = nullptr;
    unsigned *v = nullptr;
    rocprim::counting_iterator<unsigned> iota(0u);
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    if (rocprim::radix_sort_pairs(nullptr, t_sort, k, k, iota, v, m, 0, 64, stream) != hipSuccess ||
        rocprim::inclusive_scan(nullptr, t_incl, v, v, m, rocprim::plus<unsigned>(), stream) != hipSuccess ||
        rocprim::exclusive_scan(nullptr, t_excl, v, v, 0u, m + 1, rocprim::plus<unsigned>(), stream) != hipSuccess)
        GSX_FAIL("gsx_rows_decimate: rocprim size query failed");
    w->temp_bytes = std::max(t_sort, std::max(t_incl, t_excl));
    char *p = static_cast<char *>(base);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + at : nullptr;
        at += dec_align(bytes);
        return q;
    };
    w->keys0 = reinterpret_cast<unsigned long long *>(take(8 * m + 16));
    w->flag = reinterpret_cast<unsigned *>(w->keys0);
    w->nblk_in = w->flag ? w->flag + m : nullptr;
    w->keys1 = reinterpret_cast<unsigned long long *>(take(8 * m));
    w->order = reinterpret_cast<unsigned *>(take(4 * m));
    w->w = reinterpret_cast<float *>(take(4 * m));
    w->gincl = reinterpret_cast<unsigned *>(take(4 * m));
    w->heads = reinterpret_cast<unsigned *>(take(4 * (m + 1)));
    w->fsz = reinterpret_cast<unsigned *>(take(4 * m));
    w->slot = reinterpret_cast<unsigned *>(take(4 * m));
    w->item0 = reinterpret_cast<unsigned *>(take(4 * (m + 1)));
    w->longs = reinterpret_cast<unsigned *>(take(4 * (m / DEC_BLOCK + 2)));
    w->partial = reinterpret_cast<double *>(take(8 * 64 * (m / DEC_SLOT + 2)));
    w->state = reinterpret_cast<unsigned *>(take(4 * DEC_ST_WORDS));
    w->temp = take(w->temp_bytes);
    w->total = at;
    return 0;
}

// ---- (a) keys

__global__ __launch_bounds__(256) void dec_keys_kernel(const unsigned char *__restrict__ rows, int64_t first, int64_t stride, int64_t n_in,
                                                       const unsigned *__restrict__ idx, int64_t n, DecKeyArgs A,
                                                       unsigned long long *__restrict__ keys, float *__restrict__ wout,
                                                       unsigned *__restrict__ state)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    unsigned r = idx ? idx[j] : (unsigned)j;
    if ((int64_t)r >= n_in || (idx && j > 0 && idx[j - 1] >= r)) {
        atomicOr(&state[DEC_ST_STATUS], (unsigned)GSX_DECIMATE_BAD_LIST);
        r = 0u;
    }
    const int64_t b = first + (int64_t)r * stride;
    const float x = ld_f32(rows, b + A.xyz[0]), y = ld_f32(rows, b + A.xyz[1]), z = ld_f32(rows, b + A.xyz[2]);
    const float s0 = ld_f32(rows, b + A.scale[0]), s1 = ld_f32(rows, b + A.scale[1]), s2 = ld_f32(rows, b + A.scale[2]);
    const float op = ld_f32(rows, b + A.opacity);
    const double q0 = (double)ld_f32(rows, b + A.rot[0]), q1 = (double)ld_f32(rows, b + A.rot[1]);
    const double q2 = (double)ld_f32(rows, b + A.rot[2]), q3 = (double)ld_f32(rows, b + A.rot[3]);
    // splat_metric.h's expression before the negation
    const float ssum = __fadd_rn(__fadd_rn(s0, s1), s2);
    const float opa = __fdiv_rn(1.0f, __fadd_rn(1.0f, np_expf(-op)));
    const float w = __fmul_rn(np_expf(ssum), opa);
    const double qq = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3;
    const float inf = __builtin_inff();
    const bool finite_p = fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;
    const bool ok = finite_p && w > 0.0f && w < inf && qq > 0.0 && qq < (double)inf;
    unsigned long long key = (1ull << 63) | (unsigned long long)j;
    if (ok) {
        // density.hip's voxel_key, the range checked in float before the cast
        const float fx = floorf(__fdiv_rn(x, A.h)), fy = floorf(__fdiv_rn(y, A.h)), fz = floorf(__fdiv_rn(z, A.h));
        const float lo = -(float)DEC_CELL_BIAS, hi = (float)DEC_CELL_BIAS;
        if (fx >= lo && fx < hi && fy >= lo && fy < hi && fz >= lo && fz < hi) {
            const unsigned long long cx = (unsigned long long)((int)fx + DEC_CELL_BIAS), cy = (unsigned long long)((int)fy + DEC_CELL_BIAS),
                                     cz = (unsigned long long)((int)fz + DEC_CELL_BIAS);
            key = (cz << 42) | (cy << 21) | cx;
        } else {
            atomicOr(&state[DEC_ST_STATUS], (unsigned)GSX_DECIMATE_CELL_RANGE);
        }
    }
    keys[j] = key;
    wout[j] = w;
}

// ---- (c) heads, sizes, slots, blocks

__global__ __launch_bounds__(256) void dec_head_flags_kernel(const unsigned long long *__restrict__ ks, int64_t n, unsigned *__restrict__ flag)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) flag[p] = (p == 0 || ks[p] != ks[p - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void dec_head_pos_kernel(const unsigned long long *__restrict__ ks, const unsigned *__restrict__ gincl, int64_t n,
                                                           unsigned *__restrict__ heads, unsigned *__restrict__ nblk_in)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p <= n) nblk_in[p] = 0u;                          // (groups are fewer than rows: the scan's input behind the last group)
    if (p >= n) return;
    if (p == 0 || ks[p] != ks[p - 1]) heads[gincl[p] - 1u] = (unsigned)p;
    if (p == n - 1) heads[gincl[p]] = (unsigned)n;
}

__global__ __launch_bounds__(256) void dec_sizes_kernel(const unsigned long long *__restrict__ ks, const unsigned *__restrict__ gincl,
                                                        const unsigned *__restrict__ heads, const unsigned *__restrict__ order, int64_t n,
                                                        unsigned *__restrict__ fsz, unsigned *__restrict__ first_flag, unsigned *__restrict__ nblk_in,
                                                        unsigned *__restrict__ state)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool merged = false;
    if (p < n) {
        const unsigned j = order[p];
        unsigned size = 0u;
        if (p == 0 || ks[p] != ks[p - 1]) {
            const unsigned g = gincl[p] - 1u;
            size = heads[g + 1] - (unsigned)p;
            merged = size >= 2u;
            nblk_in[g] = merged ? (size + DEC_BLOCK - 1) / DEC_BLOCK : 0u;
        }
        fsz[j] = size;
        first_flag[j] = size ? 1u : 0u;
    }
    const unsigned long long bal = __ballot(merged);      // (a count: integer adds, the same whatever their order)
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&state[DEC_ST_MERGED], (unsigned)__builtin_popcountll(bal));
}

// ---- rows through LDS

// the row of `stride` bytes at byte `a` of `rows` -> LDS quads from the 16-byte boundary at or below it, by lanes l, l + nl, ...;
// -> the image's first byte inside `lds`.  Reads at most 15 bytes behind the row.
__device__ __forceinline__ int dec_stage_row(const uint4 *__restrict__ rows, int64_t a, int stride, uint4 *lds, int l, int nl)
{
    const int64_t q0 = a >> 4;
    const int nq = (int)(((a + stride + 15) >> 4) - q0);
    for (int k = l; k < nq; k += nl) lds[k] = rows[q0 + k];
    return (int)(a & 15);
}

// bytes [ib, ib + g1 - g0) of the LDS words `lds` -> bytes [g0, g1) of `out` (16-byte aligned) by lanes l, l + nl, ...: single
// bytes up to a 16-byte boundary and behind the last one, 16-byte stores between them -- nothing outside [g0, g1) is written
__device__ __forceinline__ void dec_store_row(unsigned char *__restrict__ out, int64_t g0, int64_t g1, const unsigned *lds, int ib, int l, int nl)
{
    const int64_t h = min(g1, (g0 + 15) & ~(int64_t)15);
    const int64_t tl = max(h, g1 & ~(int64_t)15);
    const int nh = (int)(h - g0), nt = (int)(g1 - tl), nb = (int)((tl - h) >> 4);
    for (int t = l; t < nh; t += nl) out[g0 + t] = (unsigned char)lds_u8(lds, ib + t);
    for (int t = l; t < nt; t += nl) out[tl + t] = (unsigned char)lds_u8(lds, ib + (int)(tl - g0) + t);
    for (int k = l; k < nb; k += nl) {
        const int o = ib + nh + 16 * k;
        uint4 v;
        v.x = lds_u32(lds, o);
        v.y = lds_u32(lds, o + 4);
        v.z = lds_u32(lds, o + 8);
        v.w = lds_u32(lds, o + 12);
        *reinterpret_cast<uint4 *>(out + h + 16 * k) = v;
    }
}

__device__ __forceinline__ void dec_lds_put32(unsigned *lds, int q, unsigned b)
{
    if ((q & 3) == 0) {
        lds[q >> 2] = b;
    } else {                                     // byte stores: a neighbouring field may share both words
        unsigned char *p = reinterpret_cast<unsigned char *>(lds) + q;
        p[0] = (unsigned char)b;
        p[1] = (unsigned char)(b >> 8);
        p[2] = (unsigned char)(b >> 16);
        p[3] = (unsigned char)(b >> 24);
    }
}

// rows that are a group of their own: 16 lanes copy one, the zeroed fields cleared in LDS on the way
__global__ __launch_bounds__(256) void dec_single_kernel(const uint4 *__restrict__ rows, int64_t first, int64_t n_in, const unsigned *__restrict__ idx,
                                                         int64_t n, const unsigned *__restrict__ fsz, const unsigned *__restrict__ slot, DecArgs A,
                                                         unsigned char *__restrict__ out, int64_t out_first)
{
    __shared__ uint4 s_row[16][DEC_ROW_QUADS];
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int64_t j = (int64_t)blockIdx.x * 16 + sub;
    const bool on = j < n && fsz[j] == 1u;
    unsigned *img = reinterpret_cast<unsigned *>(s_row[sub]);
    int ib = 0;
    if (on) {
        unsigned r = idx ? idx[j] : (unsigned)j;
        if ((int64_t)r >= n_in) r = 0u;            // (the plan call refused such a list)
        ib = dec_stage_row(rows, first + (int64_t)r * A.stride, A.stride, s_row[sub], l, 16);
    }
    __syncthreads();
    if (on)
        for (int k = l; k < A.n_zero; k += 16) dec_lds_put32(img, ib + A.zero[k], 0u);
    __syncthreads();
    if (on) {
        const int64_t g0 = out_first + (int64_t)slot[j] * A.stride;
        dec_store_row(out, g0, g0 + A.stride, img, ib, l, 16);
    }
}

// ---- (d) the terms of one member

struct DecMember {
    float x, y, z, s0, s1, s2, q0, q1, q2, q3, w;
};

// t[0 .. 10): w | w d | w (C + d d^T) in S2's order, the definition's member_terms
__device__ __forceinline__ void dec_member_terms(const DecMember &m, const double *c, double *t)
{
    const double w = (double)m.w;
    const double d0 = (double)m.x - c[0], d1 = (double)m.y - c[1], d2 = (double)m.z - c[2];
    const double a0 = (double)m.q0, a1 = (double)m.q1, a2 = (double)m.q2, a3 = (double)m.q3;
    const double qq = ((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3;
    const double nn = __dsqrt_rn(qq);
    const double qw = __ddiv_rn(a0, nn), qx = __ddiv_rn(a1, nn), qy = __ddiv_rn(a2, nn), qz = __ddiv_rn(a3, nn);
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const double xy = qx * qy, xz = qx * qz, yz = qy * qz;
    const double wx = qw * qx, wy = qw * qy, wz = qw * qz;
    const double R[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                            {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                            {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
    const double e0 = (double)np_expf(m.s0), e1 = (double)np_expf(m.s1), e2 = (double)np_expf(m.s2);
    const double v0 = e0 * e0, v1 = e1 * e1, v2 = e2 * e2;
    const double d[3] = {d0, d1, d2};
    t[0] = w;
    t[1] = w * d0;
    t[2] = w * d1;
    t[3] = w * d2;
    int i = 4;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = j; k < 3; ++k) {
            const double C = ((R[j][0] * v0) * R[k][0] + (R[j][1] * v1) * R[k][1]) + (R[j][2] * v2) * R[k][2];
            t[i++] = w * (C + d[j] * d[k]);
        }
}

// one Jacobi rotation of the pair (p, q), r the third index: the definition's jacobi3 step
__device__ __forceinline__ void dec_jacobi_rot(double &app, double &aqq, double &apq, double &arp, double &arq, double (&V)[3][3], int p, int q)
{
    if (apq == 0.0) return;
    const double theta = __ddiv_rn(aqq - app, 2.0 * apq);
    const double sgn = theta >= 0.0 ? 1.0 : -1.0;
    const double t = fabs(theta) == (double)__builtin_inff() ? 0.0 : __ddiv_rn(sgn, fabs(theta) + __dsqrt_rn(theta * theta + 1.0));
    const double c = __ddiv_rn(1.0, __dsqrt_rn(t * t + 1.0));
    const double s = t * c;
    const double napp = app - t * apq, naqq = aqq + t * apq;
    const double narp = c * arp - s * arq, narq = s * arp + c * arq;
    app = napp;
    aqq = naqq;
    apq = 0.0;
    arp = narp;
    arq = narq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = c * V[k][p] - s * V[k][q], vkq = s * V[k][p] + c * V[k][q];
        V[k][p] = vkp;
        V[k][q] = vkq;
    }
}

__device__ __forceinline__ double dec_clamp(double v, double lo, double hi)
{
    v = v < lo ? lo : v;                          // (two comparisons: a NaN stays a NaN)
    return v > hi ? hi : v;
}

struct DecGeometry {
    float pos[3], scale[3], rot[4], opacity;
};

// the group sums S[0 .. 10) and the cell centre -> the merged splat's eleven geometry fields
__device__ __noinline__ void dec_finish_geometry(const double *S, const double *c, DecGeometry *G)
{
    const double W = S[0];
    const double m0 = __ddiv_rn(S[1], W), m1 = __ddiv_rn(S[2], W), m2 = __ddiv_rn(S[3], W);
    G->pos[0] = __double2float_rn(c[0] + m0);
    G->pos[1] = __double2float_rn(c[1] + m1);
    G->pos[2] = __double2float_rn(c[2] + m2);
    double a00 = __ddiv_rn(S[4], W) - m0 * m0, a01 = __ddiv_rn(S[5], W) - m0 * m1, a02 = __ddiv_rn(S[6], W) - m0 * m2;
    double a11 = __ddiv_rn(S[7], W) - m1 * m1, a12 = __ddiv_rn(S[8], W) - m1 * m2, a22 = __ddiv_rn(S[9], W) - m2 * m2;
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < 6; ++sweep) {
        dec_jacobi_rot(a00, a11, a01, a02, a12, V, 0, 1);
        dec_jacobi_rot(a00, a22, a02, a01, a12, V, 0, 2);
        dec_jacobi_rot(a11, a22, a12, a01, a02, V, 1, 2);
    }
    const double lmin = 0x1p-126, lmax = 0x1.fffffep+127;
    const double l0 = dec_clamp(a00, lmin, lmax), l1 = dec_clamp(a11, lmin, lmax), l2 = dec_clamp(a22, lmin, lmax);
    G->scale[0] = __fmul_rn(0.5f, np_logf(__double2float_rn(l0)));
    G->scale[1] = __fmul_rn(0.5f, np_logf(__double2float_rn(l1)));
    G->scale[2] = __fmul_rn(0.5f, np_logf(__double2float_rn(l2)));
    // Shepperd: the trace, then the largest diagonal element
    const double tr = (V[0][0] + V[1][1]) + V[2][2];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        const double s = __dsqrt_rn(tr + 1.0) * 2.0;
        qw = 0.25 * s;
        qx = __ddiv_rn(V[2][1] - V[1][2], s);
        qy = __ddiv_rn(V[0][2] - V[2][0], s);
        qz = __ddiv_rn(V[1][0] - V[0][1], s);
    } else if (V[0][0] > V[1][1] && V[0][0] > V[2][2]) {
        const double s = __dsqrt_rn(((1.0 + V[0][0]) - V[1][1]) - V[2][2]) * 2.0;
        qw = __ddiv_rn(V[2][1] - V[1][2], s);
        qx = 0.25 * s;
        qy = __ddiv_rn(V[0][1] + V[1][0], s);
        qz = __ddiv_rn(V[0][2] + V[2][0], s);
    } else if (V[1][1] > V[2][2]) {
        const double s = __dsqrt_rn(((1.0 + V[1][1]) - V[0][0]) - V[2][2]) * 2.0;
        qw = __ddiv_rn(V[0][2] - V[2][0], s);
        qx = __ddiv_rn(V[0][1] + V[1][0], s);
        qy = 0.25 * s;
        qz = __ddiv_rn(V[1][2] + V[2][1], s);
    } else {
        const double s = __dsqrt_rn(((1.0 + V[2][2]) - V[0][0]) - V[1][1]) * 2.0;
        qw = __ddiv_rn(V[1][0] - V[0][1], s);
        qx = __ddiv_rn(V[0][2] + V[2][0], s);
        qy = __ddiv_rn(V[1][2] + V[2][1], s);
        qz = 0.25 * s;
    }
    const double qn = __dsqrt_rn(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = __ddiv_rn(qw, qn);
    qx = __ddiv_rn(qx, qn);
    qy = __ddiv_rn(qy, qn);
    qz = __ddiv_rn(qz, qn);
    if (qw < 0.0) {
        qw = -qw;
        qx = -qx;
        qy = -qy;
        qz = -qz;
    }
    G->rot[0] = __double2float_rn(qw);
    G->rot[1] = __double2float_rn(qx);
    G->rot[2] = __double2float_rn(qy);
    G->rot[3] = __double2float_rn(qz);
    const double alpha = __ddiv_rn(W, __dsqrt_rn((l0 * l1) * l2));
    const double ac = dec_clamp(alpha, 0x1p-24, 1.0 - 0x1p-10);
    G->opacity = np_logf(__double2float_rn(__ddiv_rn(ac, 1.0 - ac)));
}

struct DecLds {
    double geo[DEC_GEO][64];                     // the chunk's geometry terms, by member
    double sums[64];                             // the group's sums, by channel
    int64_t row[64];                             // the chunk's members: first byte of the row
    uint4 img[DEC_ROW_QUADS];                    // the output row
};

// a wave that holds a group's sums (lane c: channel c) writes the group's output row: the first member's bytes, the merged
// geometry, the averaged channels, the zeroed fields
__device__ __forceinline__ void dec_finish_group(DecLds &L, double sum, const uint4 *__restrict__ rows, int64_t first_row_byte, const double *c,
                                                 const DecArgs &A, unsigned char *__restrict__ out, int64_t out_byte)
{
    const int lane = threadIdx.x;
    L.sums[lane] = sum;
    const int ib = dec_stage_row(rows, first_row_byte, A.stride, L.img, lane, 64);
    __syncthreads();
    unsigned *img = reinterpret_cast<unsigned *>(L.img);
    const double W = L.sums[0];
    if (lane == 0) {
        double S[DEC_GEO];
#pragma unroll
        for (int k = 0; k < DEC_GEO; ++k) S[k] = L.sums[k];
        DecGeometry G;
        dec_finish_geometry(S, c, &G);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            dec_lds_put32(img, ib + A.xyz[a], __float_as_uint(G.pos[a]));
            dec_lds_put32(img, ib + A.scale[a], __float_as_uint(G.scale[a]));
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) dec_lds_put32(img, ib + A.rot[a], __float_as_uint(G.rot[a]));
        dec_lds_put32(img, ib + A.opacity, __float_as_uint(G.opacity));
    } else if (lane >= DEC_GEO && lane < DEC_GEO + A.n_mean) {
        dec_lds_put32(img, ib + A.mean[lane - DEC_GEO], __float_as_uint(__double2float_rn(__ddiv_rn(sum, W))));
    } else if (lane >= DEC_GEO + A.n_mean && lane < DEC_GEO + A.n_mean + A.n_u8) {
        double v = __builtin_rint(__ddiv_rn(sum, W));
        v = v < 0.0 ? 0.0 : v;
        v = v > 255.0 ? 255.0 : v;
        reinterpret_cast<unsigned char *>(img)[ib + A.u8[lane - DEC_GEO - A.n_mean]] = v == v ? (unsigned char)(int)v : (unsigned char)0;
    }
    __syncthreads();
    for (int k = lane; k < A.n_zero; k += 64) dec_lds_put32(img, ib + A.zero[k], 0u);
    __syncthreads();
    dec_store_row(out, out_byte, out_byte + A.stride, img, ib, lane, 64);
}

__device__ __forceinline__ void dec_cell_centre(unsigned long long key, double H, double *c)
{
    const int cx = (int)(key & 0x1fffffull) - DEC_CELL_BIAS, cy = (int)((key >> 21) & 0x1fffffull) - DEC_CELL_BIAS,
              cz = (int)((key >> 42) & 0x1fffffull) - DEC_CELL_BIAS;
    c[0] = ((double)cx + 0.5) * H;
    c[1] = ((double)cy + 0.5) * H;
    c[2] = ((double)cz + 0.5) * H;
}

__device__ __forceinline__ int64_t dec_partial_slot(unsigned head) { return ((int64_t)head + DEC_SLOT - 1) / DEC_SLOT; }

// one wave per (group, block) item
__global__ __launch_bounds__(64) void dec_sums_kernel(const uint4 *__restrict__ rows, int64_t first, int64_t n_in, const unsigned *__restrict__ idx,
                                                      unsigned groups, const unsigned long long *__restrict__ ks, const unsigned *__restrict__ order,
                                                      const float *__restrict__ wgt, const unsigned *__restrict__ heads,
                                                      const unsigned *__restrict__ item0, const unsigned *__restrict__ slot, DecArgs A,
                                                      double *__restrict__ partial, unsigned *__restrict__ longs, unsigned *__restrict__ state,
                                                      unsigned char *__restrict__ out, int64_t out_first)
{
    __shared__ DecLds L;
    const int lane = threadIdx.x;
    const unsigned t = blockIdx.x;
    // the last group whose first item is <= t: it has blocks, and t is one of them
    unsigned lo = 0u, hi = groups;                // item0[lo] <= t < item0[hi]  (item0[groups] = all items)
    while (hi - lo > 1u) {
        const unsigned mid = lo + (hi - lo) / 2u;
        if (item0[mid] <= t) lo = mid;
        else hi = mid;
    }
    const unsigned g = lo, b = t - item0[g];
    const unsigned head = heads[g], size = heads[g + 1] - head;
    const unsigned p0 = head + b * DEC_BLOCK;
    const int cnt = (int)min((unsigned)DEC_BLOCK, size - b * DEC_BLOCK);
    const unsigned char *rows8 = reinterpret_cast<const unsigned char *>(rows);
    double c[3];
    dec_cell_centre(ks[head], A.H, c);
    const int ch = lane - DEC_GEO;
    const int off = ch >= 0 && ch < A.n_mean ? A.mean[ch] : (ch >= A.n_mean && ch < A.n_mean + A.n_u8 ? A.u8[ch - A.n_mean] : -1);
    const bool is_u8 = ch >= A.n_mean;
    double acc = 0.0;
    for (int m0 = 0; m0 < cnt; m0 += 64) {
        const int cm = min(64, cnt - m0);
        __syncthreads();
        if (lane < cm) {
            const unsigned j = order[p0 + m0 + lane];
            unsigned r = idx ? idx[j] : j;
            if ((int64_t)r >= n_in) r = 0u;        // (the plan call refused such a list)
            const int64_t a = first + (int64_t)r * A.stride;
            DecMember M;
            M.x = ld_f32(rows8, a + A.xyz[0]);
            M.y = ld_f32(rows8, a + A.xyz[1]);
            M.z = ld_f32(rows8, a + A.xyz[2]);
            M.s0 = ld_f32(rows8, a + A.scale[0]);
            M.s1 = ld_f32(rows8, a + A.scale[1]);
            M.s2 = ld_f32(rows8, a + A.scale[2]);
            M.q0 = ld_f32(rows8, a + A.rot[0]);
            M.q1 = ld_f32(rows8, a + A.rot[1]);
            M.q2 = ld_f32(rows8, a + A.rot[2]);
            M.q3 = ld_f32(rows8, a + A.rot[3]);
            M.w = wgt[j];
            double tm[DEC_GEO];
            dec_member_terms(M, c, tm);
#pragma unroll
            for (int k = 0; k < DEC_GEO; ++k) L.geo[k][lane] = tm[k];
            L.row[lane] = a;
        }
        __syncthreads();
        if (lane < DEC_GEO) {
            for (int m = 0; m < cm; ++m) acc = acc + L.geo[lane][m];
        } else if (off >= 0) {
            if (is_u8) {
                for (int m = 0; m < cm; ++m) acc = acc + L.geo[0][m] * (double)rows8[L.row[m] + off];
            } else {
#pragma unroll 4
                for (int m = 0; m < cm; ++m) acc = acc + L.geo[0][m] * (double)ld_f32(rows8, L.row[m] + off);
            }
        }
    }
    if (size > (unsigned)DEC_BLOCK) {
        partial[(dec_partial_slot(head) + b) * 64 + lane] = acc;
        if (b == 0u && lane == 0) longs[atomicAdd(&state[DEC_ST_LONG], 1u)] = g;   // (a list of independent groups: its order is not used)
        return;
    }
    const unsigned j0 = order[head];
    unsigned r0 = idx ? idx[j0] : j0;
    if ((int64_t)r0 >= n_in) r0 = 0u;
    __syncthreads();
    dec_finish_group(L, acc, rows, first + (int64_t)r0 * A.stride, c, A, out, out_first + (int64_t)slot[j0] * A.stride);
}

// one wave per group above 256 rows: its blocks' partial sums in block order, then the finish
__global__ __launch_bounds__(64) void dec_long_kernel(const uint4 *__restrict__ rows, int64_t first, int64_t n_in, const unsigned *__restrict__ idx,
                                                      const unsigned long long *__restrict__ ks, const unsigned *__restrict__ order,
                                                      const unsigned *__restrict__ heads, const unsigned *__restrict__ slot, DecArgs A,
                                                      const double *__restrict__ partial, const unsigned *__restrict__ longs,
                                                      const unsigned *__restrict__ state, unsigned char *__restrict__ out, int64_t out_first)
{
    __shared__ DecLds L;
    if (blockIdx.x >= state[DEC_ST_LONG]) return;
    const int lane = threadIdx.x;
    const unsigned g = longs[blockIdx.x];
    const unsigned head = heads[g], size = heads[g + 1] - head;
    const unsigned nb = (size + DEC_BLOCK - 1) / DEC_BLOCK;
    const int64_t q0 = dec_partial_slot(head);
    double acc = 0.0;
    for (unsigned b0 = 0; b0 < nb; b0 += 16) {          // sixteen loads in flight, added in block order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = partial[(q0 + min(b0 + u, nb - 1)) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (b0 + u < nb) acc = acc + v[u];
    }
    double c[3];
    dec_cell_centre(ks[head], A.H, c);
    const unsigned j0 = order[head];
    unsigned r0 = idx ? idx[j0] : j0;
    if ((int64_t)r0 >= n_in) r0 = 0u;
    dec_finish_group(L, acc, rows, first + (int64_t)r0 * A.stride, c, A, out, out_first + (int64_t)slot[j0] * A.stride);
}

// gsx_decimate_layout -> the kernels' arguments: every field inside a row, the voxel size a finite number above 0
static int dec_args(const gsx_decimate_layout *l, int64_t stride, DecArgs *A, DecKeyArgs *K, const char *who)
{
    if (!l) GSX_FAIL("%s: null layout", who);
    if (!(l->voxel_size > 0.0) || !(l->voxel_size < (double)__builtin_inff())) GSX_FAIL("%s: a voxel size of %g (a finite number above 0)", who, l->voxel_size);
    if (l->n_mean < 0 || l->n_mean > GSX_DECIMATE_MAX_MEAN || (l->n_u8 != 0 && l->n_u8 != 3) || l->n_zero < 0 || l->n_zero > GSX_DECIMATE_MAX_ZERO)
        GSX_FAIL("%s: %d averaged fields (0 ... %d), %d colour bytes (0 or 3), %d zeroed fields (0 ... %d)", who, l->n_mean, GSX_DECIMATE_MAX_MEAN, l->n_u8,
                 l->n_zero, GSX_DECIMATE_MAX_ZERO);
    memset(A, 0, sizeof(*A));
    A->H = l->voxel_size;
    A->stride = (int)stride;
    A->n_mean = l->n_mean;
    A->n_u8 = l->n_u8;
    A->n_zero = l->n_zero;
    auto inside = [&](int o, int bytes, const char *what, int k) -> int {
        if (o < 0 || o + bytes > stride) GSX_FAIL("%s: %s field %d at byte offset %d of a %lld-byte row", who, what, k, o, (long long)stride);
        return 0;
    };
    for (int a = 0; a < 3; ++a) {
        GSX_CHECK(inside(l->xyz_offset[a], 4, "position", a));
        GSX_CHECK(inside(l->scale_offset[a], 4, "scale", a));
        A->xyz[a] = K->xyz[a] = l->xyz_offset[a];
        A->scale[a] = K->scale[a] = l->scale_offset[a];
    }
    for (int a = 0; a < 4; ++a) {
        GSX_CHECK(inside(l->rot_offset[a], 4, "rotation", a));
        A->rot[a] = K->rot[a] = l->rot_offset[a];
    }
    GSX_CHECK(inside(l->opacity_offset, 4, "opacity", 0));
    A->opacity = K->opacity = l->opacity_offset;
    K->h = (float)l->voxel_size;
    for (int k = 0; k < l->n_mean; ++k) {
        GSX_CHECK(inside(l->mean_offset[k], 4, "averaged", k));
        A->mean[k] = (short)l->mean_offset[k];
    }
    for (int k = 0; k < l->n_u8; ++k) {
        GSX_CHECK(inside(l->u8_offset[k], 1, "colour", k));
        A->u8[k] = (short)l->u8_offset[k];
    }
    const int32_t geo[11] = {l->xyz_offset[0], l->xyz_offset[1], l->xyz_offset[2], l->scale_offset[0], l->scale_offset[1], l->scale_offset[2],
                             l->rot_offset[0], l->rot_offset[1], l->rot_offset[2], l->rot_offset[3], l->opacity_offset};
    for (int k = 0; k < l->n_zero; ++k) {
        const int o = l->zero_offset[k];
        GSX_CHECK(inside(o, 4, "zeroed", k));
        for (int f = 0; f < 11; ++f)
            if (o < geo[f] + 4 && geo[f] < o + 4) GSX_FAIL("%s: zeroed field %d at byte offset %d overlaps a geometry field", who, k, o);
        A->zero[k] = (short)o;
    }
    return 0;
}

static int dec_common(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n_in, const uint32_t *idx_dev, int64_t n,
                      const void *work_dev, const char *who)
{
    if (!c || (n > 0 && (!rows_dev || !work_dev))) GSX_FAIL("%s: null argument", who);
    if (n_in < 0 || n_in >= (1LL << 32) || n < 0 || n > n_in || n >= (1LL << 31) || (!idx_dev && n != n_in))
        GSX_FAIL("%s: %lld of %lld rows (without a list: all of them; fewer than 2^31)", who, (long long)n, (long long)n_in);
    GSX_CHECK(rows_args(rows_dev, first_byte, stride, who));
    if ((reinterpret_cast<uintptr_t>(work_dev) & 15) || (reinterpret_cast<uintptr_t>(idx_dev) & 3))
        GSX_FAIL("%s: the workspace must be 16-byte aligned, the list 4-byte aligned", who);
    return 0;
}

// stream clocks of consecutive stages: mark() after each, read() joins the stream and adds the milliseconds between the marks
struct DecClock {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int used = 0;
    bool on;
    hipStream_t stream;
    DecClock(bool on_, hipStream_t s) : on(on_), stream(s) {}
    ~DecClock()
    {
        for (int k = 0; k < 4; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
    int mark()
    {
        if (!on) return 0;
        GSX_HIP(hipEventCreate(&ev[used]));
        GSX_HIP(hipEventRecord(ev[used], stream));
        ++used;
        return 0;
    }
    int read(float *into)
    {
        if (!on) return 0;
        GSX_HIP(hipStreamSynchronize(stream));
        for (int k = 0; k + 1 < used; ++k) {
            float ms = 0.0f;
            GSX_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            into[k] += ms;
        }
        return 0;
    }
};

}  // namespace gsx

using namespace gsx;

extern "C" {

int gsx_rows_decimate_work_dev(gsx_ctx *c, int64_t n, int64_t *bytes_out)
{
    if (!c || !bytes_out) GSX_FAIL("gsx_rows_decimate_work_dev: null argument");
    if (n < 0 || n >= (1LL << 31)) GSX_FAIL("gsx_rows_decimate_work_dev: %lld rows (fewer than 2^31)", (long long)n);
    GSX_HIP(hipSetDevice(c->device));
    DecWs w;
    GSX_CHECK(dec_carve(n, nullptr, c->stream, &w));
    *bytes_out = (int64_t)w.total;
    return 0;
}

int gsx_rows_decimate_plan_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n_in, const uint32_t *idx_dev,
                               int64_t n, const gsx_decimate_layout *layout, void *work_dev, int64_t work_bytes, int64_t *info_out, float *stage_ms)
{
    const char *who = "gsx_rows_decimate_plan_dev";
    if (!info_out) GSX_FAIL("%s: null argument", who);
    GSX_CHECK(dec_common(c, rows_dev, first_byte, stride, n_in, idx_dev, n, work_dev, who));
    DecArgs A;
    DecKeyArgs K;
    GSX_CHECK(dec_args(layout, stride, &A, &K, who));
    for (int k = 0; k < GSX_DECIMATE_INFO_WORDS; ++k) info_out[k] = 0;
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0) return 0;
    DecWs w;
    GSX_CHECK(dec_carve(n, work_dev, c->stream, &w));
    if ((int64_t)w.total > work_bytes) GSX_FAIL("%s: a workspace of %lld bytes, %zu are needed", who, (long long)work_bytes, w.total);
    const unsigned blocks = (unsigned)((n + 255) / 256), blocks1 = (unsigned)((n + 1 + 255) / 256);
    const unsigned char *rows8 = static_cast<const unsigned char *>(rows_dev);
    DecClock clock(stage_ms != nullptr, c->stream);
    GSX_HIP(hipMemsetAsync(w.state, 0, 4 * DEC_ST_WORDS, c->stream));
    GSX_CHECK(clock.mark());
    hipLaunchKernelGGL(dec_keys_kernel, dim3(blocks), dim3(256), 0, c->stream, rows8, first_byte, stride, n_in, idx_dev, n, K, w.keys0, w.w, w.state);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(clock.mark());
    rocprim::counting_iterator<unsigned> iota(0u);
    size_t tb = w.temp_bytes;
    GSX_HIP(rocprim::radix_sort_pairs(w.temp, tb, w.keys0, w.keys1, iota, w.order, (size_t)n, 0, 64, c->stream));   // stable
    GSX_CHECK(clock.mark());
    hipLaunchKernelGGL(dec_head_flags_kernel, dim3(blocks), dim3(256), 0, c->stream, w.keys1, n, w.flag);
    tb = w.temp_bytes;
    GSX_HIP(rocprim::inclusive_scan(w.temp, tb, w.flag, w.gincl, (size_t)n, rocprim::plus<unsigned>(), c->stream));
    hipLaunchKernelGGL(dec_head_pos_kernel, dim3(blocks1), dim3(256), 0, c->stream, w.keys1, w.gincl, n, w.heads, w.nblk_in);
    hipLaunchKernelGGL(dec_sizes_kernel, dim3(blocks), dim3(256), 0, c->stream, w.keys1, w.gincl, w.heads, w.order, n, w.fsz, w.flag, w.nblk_in,
                       w.state);
    GSX_HIP(hipGetLastError());
    tb = w.temp_bytes;
    GSX_HIP(rocprim::exclusive_scan(w.temp, tb, w.flag, w.slot, 0u, (size_t)n, rocprim::plus<unsigned>(), c->stream));
    tb = w.temp_bytes;
    GSX_HIP(rocprim::exclusive_scan(w.temp, tb, w.nblk_in, w.item0, 0u, (size_t)n + 1, rocprim::plus<unsigned>(), c->stream));
    GSX_CHECK(clock.mark());
    unsigned state[DEC_ST_WORDS] = {0, 0, 0, 0}, groups = 0, items = 0;
    GSX_HIP(hipMemcpyAsync(state, w.state, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipMemcpyAsync(&groups, w.gincl + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipMemcpyAsync(&items, w.item0 + n, 4, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if (stage_ms) GSX_CHECK(clock.read(stage_ms));
    info_out[0] = (state[DEC_ST_STATUS] & GSX_DECIMATE_BAD_LIST) ? GSX_DECIMATE_BAD_LIST : (state[DEC_ST_STATUS] ? GSX_DECIMATE_CELL_RANGE : GSX_DECIMATE_OK);
    info_out[1] = groups;
    info_out[2] = state[DEC_ST_MERGED];
    info_out[3] = items;
    info_out[4] = (int64_t)groups - (int64_t)state[DEC_ST_MERGED];
    return 0;
}

int gsx_rows_decimate_write_dev(gsx_ctx *c, const void *rows_dev, int64_t first_byte, int64_t stride, int64_t n_in, const uint32_t *idx_dev,
                                int64_t n, const gsx_decimate_layout *layout, void *work_dev, int64_t work_bytes, void *out_dev,
                                int64_t out_first_byte, int64_t n_out, float *stage_ms)
{
    const char *who = "gsx_rows_decimate_write_dev";
    GSX_CHECK(dec_common(c, rows_dev, first_byte, stride, n_in, idx_dev, n, work_dev, who));
    if (n_out < 0 || n_out > n || (n_out > 0 && !out_dev)) GSX_FAIL("%s: %lld output rows for %lld rows", who, (long long)n_out, (long long)n);
    GSX_CHECK(rows_args(out_dev, out_first_byte, stride, who, "output rows"));
    DecArgs A;
    DecKeyArgs K;
    GSX_CHECK(dec_args(layout, stride, &A, &K, who));
    GSX_HIP(hipSetDevice(c->device));
    if (n == 0 || n_out == 0) return 0;
    DecWs w;
    GSX_CHECK(dec_carve(n, work_dev, c->stream, &w));
    if ((int64_t)w.total > work_bytes) GSX_FAIL("%s: a workspace of %lld bytes, %zu are needed", who, (long long)work_bytes, w.total);
    // the plan's own counts, read again: the launches below are sized by them, not by the caller's word
    unsigned groups = 0, items = 0;
    GSX_HIP(hipMemcpyAsync(&groups, w.gincl + (n - 1), 4, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipMemcpyAsync(&items, w.item0 + n, 4, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(hipStreamSynchronize(c->stream));
    if ((int64_t)groups != n_out) GSX_FAIL("%s: %lld output rows, the plan in the workspace has %u", who, (long long)n_out, groups);
    const uint4 *rows4 = static_cast<const uint4 *>(rows_dev);
    unsigned char *out8 = static_cast<unsigned char *>(out_dev);
    DecClock clock(stage_ms != nullptr, c->stream);
    GSX_HIP(hipMemsetAsync(w.state + DEC_ST_LONG, 0, 4, c->stream));
    GSX_CHECK(clock.mark());
    if (items)
        hipLaunchKernelGGL(dec_sums_kernel, dim3(items), dim3(64), 0, c->stream, rows4, first_byte, n_in, idx_dev, groups, w.keys1, w.order, w.w, w.heads,
                           w.item0, w.slot, A, w.partial, w.longs, w.state, out8, out_first_byte);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(clock.mark());
    if (items)
        hipLaunchKernelGGL(dec_long_kernel, dim3((unsigned)(n / DEC_BLOCK + 1)), dim3(64), 0, c->stream, rows4, first_byte, n_in, idx_dev, w.keys1, w.order,
                           w.heads, w.slot, A, w.partial, w.longs, w.state, out8, out_first_byte);
    hipLaunchKernelGGL(dec_single_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, c->stream, rows4, first_byte, n_in, idx_dev, n, w.fsz, w.slot, A,
                       out8, out_first_byte);
    GSX_HIP(hipGetLastError());
    GSX_CHECK(clock.mark());
    if (stage_ms) GSX_CHECK(clock.read(stage_ms + 3));
    return 0;
}

}  // extern "C"
