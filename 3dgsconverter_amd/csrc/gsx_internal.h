// gsx_internal.h -- every function one .hip file defines and another calls, declared once.  The defining file includes this
// header too, so a signature that drifts is a compile error there.  (Functions of the C ABI are declared in include/gsx_hip.h.)
#pragma once

#include "gsx_common.h"

namespace gsx {

struct SlabKnn;   // sor_grid_params.h

// ---- sor_brute.hip
// SoA columns -> float4 rows; flags non-finite input in ctx->devflags
int launch_pack_points(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n, float4 *out);
int launch_knn_brute(gsx_ctx *ctx, const float4 *pts, int64_t n_ref, int64_t q_begin, int64_t q_count, const unsigned *qlist,
                     const unsigned *qlist_count, int64_t qlist_cap, int k, float *mean_out);

// ---- sor_grid.hip
int launch_knn_grid(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n_ref, int64_t q_begin,
                    int64_t q_count, int k, float *mean_out, gsx_sor_info *info, int share = 0, int nshares = 1);
// Multi-GPU slab: points [0, n_own) are queries, [n_own, n_own + n_halo) reference-only; kth_out (nullable) receives
// every query's (k+1)-th squared distance so that the caller can certify it against the slab's open faces.
int launch_knn_slab(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n_own, int64_t n_halo,
                    int k, float *mean_out, double *kth_out, const SlabKnn *sk = nullptr);

// ---- sor_tree.hip: the path for clouds the grid cannot resolve
int launch_knn_tree(gsx_ctx *ctx, const float *x, const float *y, const float *z, int64_t stride, int64_t n_ref, int64_t q_begin,
                    int64_t q_count, int k, float *mean_out, double *kth_out, gsx_sor_info *info, int64_t ref_only_from, int share,
                    int nshares, bool guard);
int knn_tree_info(gsx_ctx *ctx, gsx_sor_info *info);
int knn_tree_debug(gsx_ctx *ctx, uint32_t *counters, uint64_t *keys, uint32_t *leafstart, int64_t cap, int64_t *n_out,
                   int64_t *leaves_out);

// ---- sor_stats.hip
int launch_sor_stats(gsx_ctx *ctx, const float *md, int64_t n, double factor, float *stats_dev);
int launch_sor_mask(gsx_ctx *ctx, const float *md, int64_t n, const float *thr_dev, uint8_t *mask);
int launch_sor_piece_sums(gsx_ctx *ctx, const float *a, int64_t n, const float *mean_dev, float *piece_out);
int launch_sor_stats_from_pieces(gsx_ctx *ctx, const float *pieces, int64_t npieces, int64_t n_total, int mode, double factor,
                                 float *stats_dev);

// ---- density.hip
int density_voxels_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                       int64_t min_points, int64_t dense_cap, int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                       int64_t *dense_counts_out);
int density_hist_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                     int64_t cap, int64_t *n_unique_out, int64_t *keys3_dev, int64_t *counts_dev);
int density_merge_dev(gsx_ctx *c, const int64_t *keys3_dev, const int64_t *counts_dev, int64_t m, int64_t min_points,
                      int64_t dense_cap, int64_t *n_unique_out, int64_t *n_dense_out, int64_t *dense_keys_out,
                      int64_t *dense_counts_out);
int density_mask_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                     const int64_t *kept_keys, int64_t n_kept, uint8_t *mask_dev);
int density_filter_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n, double voxel_size,
                       int64_t min_points, int keep_multi, const float *box6, uint8_t *mask_dev, gsx_density_info *info);
int density_filter_large_dev(gsx_ctx *c, const float *x, const float *y, const float *z, int64_t stride, int64_t n,
                             double voxel_size, int64_t min_points, int keep_multi, const float *box6, uint8_t *mask_dev,
                             gsx_density_info *info);
int voxel_clusters_dev(gsx_ctx *c, const int64_t *keys3, int64_t m, int keep_multi, uint8_t *keep_out, gsx_density_info *info);

// ---- kmeans.hip
int kmeans_lloyd_dev(gsx_ctx *c, const float *data_dev, int64_t n, int d, int k, int max_iter, float *cent_dev, int32_t *labels_dev);
int kmeans_lloyd_batch_dev(gsx_ctx *c, const float *data_dev, const int64_t *off_host, int nprob, int d, int k, int max_iter,
                           float *cent_dev, int32_t *labels_dev);
int quantize_dev(gsx_ctx *c, const float *vals_dev, int64_t n, const float *cb_dev, int kcb, uint8_t *out_dev);

}  // namespace gsx
