/* h3d.h — C ABI of libh3d.so, the MI355X-native hot path of hic3defdr.
 *
 * The reference (thomasgilgenast/hic3defdr 0.2.1) is pure Python and has no
 * FFI; this ABI sits behind its operator-level functions, which the Python
 * mirror (hic3defdr_amd) binds with ctypes:
 *
 *   h3d_union_*            <- util/matrices.py:92-129 sparse_union (+ the raw /
 *                              balanced gathers, analysis/analysis.py:91-101)
 *   h3d_size_factors_cmor  <- util/scaling.py:108-127 conditional_mor
 *   h3d_size_factors       <- util/scaling.py:10-149 (every norm prepare_data
 *                              dispatches, analysis/analysis.py:104-108)
 *   h3d_disp_per_dist      <- analysis/analysis.py:185-206 (estimator per
 *                              distance/condition; util/dispersion.py:10-80
 *                              qcml/cml, util/scaled_nb.py:71-275)
 *   h3d_disp_table         <- analysis/analysis.py:208-218 +
 *                              util/lowess.py:10-244 (the fitted disp_fn,
 *                              tabulated on every integer distance)
 *   h3d_lrt                <- util/lrt.py:7-50 (+ analysis/analysis.py:272-278)
 *   h3d_lrt_wide           <- util/lrt.py:7 lrt(raw, f, disp, design) as called
 *   h3d_cml                <- util/dispersion.py:46-80 cml
 *   h3d_nb_fit_mu / _dev   <- util/scaled_nb.py:71-183 fit_mu_hat
 *   h3d_nb_equalize / _dev <- util/scaled_nb.py:186-214 equalize
 *   h3d_nb_quantile_map    <- util/scaled_nb.py:217-275 q2qnbinom
 *   h3d_nb_logpmf          <- util/scaled_nb.py:12-33 logpmf
 *   h3d_nb_sample / _dev   <- util/simulation.py:187-203 (the negative-binomial
 *                              draw of one replicate; a counter-based stream)
 *   h3d_simulate_dev       <- util/simulation.py:187-203, every replicate of a
 *                              chromosome from the means, biases, size factors
 *   h3d_bh / _ctx / _dev   <- analysis/analysis.py:286-303 (lib5c
 *                              adjust_pvalues = BH)
 *   h3d_find_clusters      <- util/clusters.py:73-97 find_clusters (threshold /
 *                              classify, analysis.py:366-486)
 *   h3d_label_components / _dev, h3d_cluster_lists / _dev
 *                          <- util/clusters.py:69-97 as connected components
 *                              (threshold / classify with gpu=True)
 *   h3d_threshold_classes_dev <- util/thresholding.py:7-41 (q < fdr, q >= fdr)
 *   h3d_argmax_classes_dev <- util/classification.py:7-49 (np.argmax)
 *   h3d_cluster_stats / _dev <- util/cluster_table.py:192-332
 *                              add_columns_to_cluster_table (mean / max / min
 *                              of a sparse table over every cluster's pixels)
 *   h3d_format_clusters    <- util/clusters.py:129-130 save_clusters text,
 *                              util/cluster_table.py:67 "cluster" column
 *   h3d_lrt_poisson        <- analysis/alternatives.py:17-42 poisson_lrt
 *                              (Poisson3DeFDR.lrt, :73-115)
 *   h3d_mme_per_pixel      <- util/dispersion.py:83-104 mme_per_pixel
 *                              (Unsmoothed3DeFDR.estimate_disp,
 *                              alternatives.py:119-137)
 *   h3d_window_gather      <- util/matrices.py:132-160 select_matrix,
 *                              analysis/core.py:255-291 get_matrix,
 *                              util/apa.py:6-44 make_apa_stack
 *   h3d_stack_aggregate    <- np.nanmean over an APA stack (docs/apa.rst)
 *   h3d_filter_sparse_rows <- util/filtering.py:8-33 filter_sparse_rows_count
 *   h3d_kr_balance         <- util/balancing.py:5-208 kr_balance (behind the
 *                              filter: README.md:602-614)
 *   h3d_group_sums / _dev  <- plotting/distance_dependence.py:34-43 (the sums
 *                              per distance bin), plotting/dispersion.py:133-144,
 *                              :182-183 (the means per distance)
 *   h3d_histogram / _dev   <- plotting/histograms.py (plt.hist = np.histogram;
 *                              analysis/plotting.py:200-249)
 *   h3d_ma_stats           <- analysis/plotting.py:307, plotting/ma.py:71-72,
 *                              :131-155 (means, M, A, the series of each pixel)
 *   h3d_density_grid       <- the ax.scatter_density calls of plotting/ma.py
 *                              as per-class np.histogram2d counts
 *   h3d_rank_average       <- scipy.stats.rankdata under spearmanr
 *                              (analysis/plotting.py:369-376)
 *   h3d_corr_matrix        <- scipy.stats.pearsonr / spearmanr over replicate
 *                              pairs (analysis/plotting.py:369-376)
 *   h3d_pixel_moments      <- analysis/plotting.py:128-129 np.mean / np.var
 *   h3d_balance_pixels     <- analysis/plotting.py:46-48 balanced
 *
 * Conventions: 0 on success, a negative H3D_E* code otherwise (the message is
 * in h3d_last_error(), thread-local). Host buffers are C-contiguous and owned
 * by the caller; device buffers of the *_dev entry points are device pointers
 * the caller owns. Calls are synchronous unless they take a stream. One ctx
 * per device; a ctx is not shared between threads.
 */
#ifndef H3D_H_
#define H3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H3D_OK 0
#define H3D_EARG (-1)    /* bad argument: null pointer, size, shape        */
#define H3D_EHIP (-2)    /* HIP runtime error                               */
#define H3D_ENOCONV (-3) /* numerical failure the reference raises on      */
#define H3D_ENOMEM (-4)  /* device allocation failed                       */
#define H3D_EINPUT (-5)  /* invalid numeric input (reference asserts)      */
#define H3D_ENODEV (-6)  /* no usable gfx950 device                        */

#define H3D_EST_QCML 0
#define H3D_EST_CML 1
#define H3D_EST_MME 2

/* size-factor methods (util/scaling.py) */
#define H3D_NORM_CONDITIONAL_MOR 0     /* :108-127, (n, R)                */
#define H3D_NORM_CONDITIONAL_SCALING 1 /* :130-149, (n, R)                */
#define H3D_NORM_MEDIAN_OF_RATIOS 2    /* :27-47, (R,)                    */
#define H3D_NORM_SIMPLE_SCALING 3      /* :50-65, (R,)                    */
#define H3D_NORM_NO_SCALING 4          /* :10-24, (R,)                    */

/* per-segment / per-pixel status bits (also in *flags outputs) */
#define H3D_FLAG_NOROOT 1   /* all-zero counts: no MLE (ref ValueError)      */
#define H3D_FLAG_NOCONV 2   /* MLE solver did not converge                   */
#define H3D_FLAG_BRENT 4    /* bounded Brent failed (ref assert res.success) */
#define H3D_FLAG_QGUARD 8   /* qcml did not converge in 1000 iterations      */
#define H3D_FLAG_BADIN 16   /* alpha/b not positive finite (ref assert)      */

typedef struct h3d_ctx h3d_ctx;

/* All-reduce hook for multi-GPU estimate_disp: called between data passes
 * with a DEVICE buffer of `count` doubles that must be summed in place across
 * ranks on the ctx stream (e.g. torch.distributed.all_reduce over RCCL).
 * Return 0 on success. */
typedef int (*h3d_allreduce_fn)(double* dev_buf, int64_t count, void* user);

int h3d_version(void);
int h3d_device_count(void);
h3d_ctx* h3d_open(int device);
void h3d_close(h3d_ctx* ctx);
const char* h3d_last_error(void);
/* stream the ctx launches on (hipStream_t); NULL = the ctx's own stream */
int h3d_set_stream(h3d_ctx* ctx, void* stream);
/* qcml's convergence tolerance for the ctx's later estimate_disp calls
 * (util/dispersion.py:10-43 qcml(..., tol=1e-4): iterate while
 * |disp - new disp| > tol); default 1e-4, the value the reference's
 * estimate_disp uses. H3D_EARG for a negative or non-finite tol. */
int h3d_set_qcml_tol(h3d_ctx* ctx, double tol);

/* ---- prepare_data ------------------------------------------------------ */

/* Native reader of the replicate contact matrices: scipy.sparse.save_npz
 * archives as the reference loads them with scipy.sparse.load_npz
 * (analysis/analysis.py:94,100 through util/matrices.py:122-124). Host only,
 * no context. _info reads the archive's directory and the shape / format /
 * data headers; _read inflates indptr, indices and data (libdeflate when
 * the system has libdeflate.so.0, else zlib; one thread each) into caller
 * buffers of n_rows + 1, nnz, nnz entries, converting to
 * int64 / int32 / float64, and sets *canonical = 1 when every row's columns
 * are strictly increasing (the layout h3d_union_count takes as is). H3D_EARG
 * for a missing file, a non-CSR archive or an unsupported dtype. */
int h3d_npz_csr_info(const char* path, int64_t* n_rows, int64_t* n_cols,
                     int64_t* nnz);
int h3d_npz_csr_read(const char* path, int64_t n_rows, int64_t nnz,
                     int64_t* indptr, int32_t* indices, double* data,
                     int* canonical);
/* The same, with `slack` writable bytes before `indices` and before `data`:
 * a member of the target's width (little-endian int32 indices; 8-byte data:
 * float64, or int64 / uint64 converted in place) whose .npy header fits in
 * the slack is inflated in place (the header lands in the slack), with no
 * scratch copy. slack 0 = h3d_npz_csr_read. */
int h3d_npz_csr_read_slack(const char* path, int64_t n_rows, int64_t nnz,
                           int64_t* indptr, int32_t* indices, double* data,
                           int64_t slack, int* canonical);
/* 1 when the reader inflates through libdeflate, 0 through zlib. */
int h3d_npz_backend(void);
/* A one-column text file as np.loadtxt reads it -- load_bias's bias vectors
 * (core.py:35-60: np.loadtxt per replicate file): one number per line, blank
 * lines and '#' comments skipped, values by strtod (correctly rounded, as
 * numpy's parser). *n = the values written to out (capacity cap). H3D_EINPUT
 * for any line that is not exactly one decimal number (the caller then reads
 * the file with np.loadtxt and its errors); H3D_EARG for a missing file or
 * more than cap values. Host only. */
int h3d_read_text_column(const char* path, double* out, int64_t cap, int64_t* n);

/* Union pixel set of R upper-triangular CSR replicate matrices restricted to
 * 0 <= col-row <= dist_max and to bins whose bias is non-zero in every
 * replicate (matrices.py:92-129 with deconvolute(invert=True)). Two-pass:
 * count, then fill. indptr[r] has n_bins+1 entries, indices[r]/data[r] nnz[r].
 * bias is (n_bins, R) row-major and already bias_thresh-filtered
 * (core.py:35-60). */
int h3d_union_count(h3d_ctx* ctx, int R, int n_bins, const int64_t* const* indptr,
                    const int32_t* const* indices, const double* const* data,
                    const int64_t* nnz, const double* bias, int dist_max,
                    int64_t* n_px_out);
/* row/col (n_px), raw (n_px, R) int64 = summed counts, balanced (n_px, R) =
 * raw / (bias[row, r] * bias[col, r]) (analysis.py:91-101). */
int h3d_union_fill(h3d_ctx* ctx, int32_t* row, int32_t* col, int64_t* raw,
                   double* balanced, int64_t n_px);
/* h3d_union_fill that also leaves the union in caller-owned DEVICE buffers
 * (each may be NULL): d_row / d_col (n_px) int32, d_raw (n_px, R) int32 --
 * H3D_EINPUT, after the host outputs are written, if a count does not fit
 * --, d_balanced (n_px, R). The host `balanced` may be NULL when d_balanced
 * is not (the device computes scaled from it, h3d_scale_disp_dev), the host
 * `raw` when d_raw is not (the caller fetches it in the background). The
 * product keeps a chromosome resident this way between prepare_data and
 * estimate_disp / lrt (analysis.py:128-133 writes the same arrays to the
 * outdir, :169-183 and :261-275 read them back). */
int h3d_union_fill_dev(h3d_ctx* ctx, int32_t* row, int32_t* col, int64_t* raw,
                       double* balanced, int64_t n_px, int32_t* d_row,
                       int32_t* d_col, int32_t* d_raw, double* d_balanced);

/* Distance-conditional median-of-ratios size factors (scaling.py:68-127) with
 * n_bins equal-number distance bins (stable tie order), or
 * exact distances when n_bins == 0. balanced (n, R), dist (n) -> sf (n, R). */
int h3d_size_factors_cmor(h3d_ctx* ctx, const double* balanced,
                          const int32_t* dist, int64_t n, int R, int n_bins,
                          double* sf_out);

/* Size factors of any norm (scaling.py): the conditional methods condition
 * on distance (n_bins equal-number bins, or exact distances when n_bins ==
 * 0; scaling.py:68-105) and write sf (n, R); the global ones write one
 * factor per replicate, sf (R). balanced (n, R), dist (n; unused by the
 * global methods, may be NULL). */
int h3d_size_factors(h3d_ctx* ctx, const double* balanced, const int32_t* dist,
                     int64_t n, int R, int norm, int n_bins, double* sf_out);
/* The same on a DEVICE balanced (n, R) (h3d_union_fill_dev's), dist (n) on
 * the host; sf on the host as h3d_size_factors writes it and, when d_sf_out
 * is not NULL, in that device buffer too ((n, R) or (R,)); sf_out may be
 * NULL for the conditional norms when d_sf_out is given. */
int h3d_size_factors_dev(h3d_ctx* ctx, const double* d_balanced,
                         const int32_t* dist, int64_t n, int R, int norm,
                         int n_bins, double* sf_out, double* d_sf_out);

/* prepare_data's scaled and disp_idx on the device (analysis.py:109-115,
 * replaces the host `balanced / size_factors`, `np.dot(scaled, design) /
 * n_c` and `np.all(mean >= mean_thresh, axis=1) & (dist >= dist_thresh_min)`):
 * d_balanced (n, R) and d_sf ((n, R), or (R,) with sf_per_rep) on the device,
 * design (R, C) 0/1 row-major on the host. Writes scaled (n, R) and flag (n)
 * to the host and, when d_flag_out / d_scaled_out are not NULL, flag /
 * scaled to those device buffers (scaled_out may then be NULL).
 * flag = 1 / 0 is disp_idx; 2 marks a row whose decision could depend on the
 * product's summation order (a non-finite scaled value, or a mean within
 * 1e-12 relative of mean_thresh): the caller decides those rows with numpy's
 * product. Synchronous. */
int h3d_scale_disp_dev(h3d_ctx* ctx, const double* d_balanced, const double* d_sf,
                       int sf_per_rep, const int32_t* d_row, const int32_t* d_col, int64_t n,
                       int R, int C, const uint8_t* design, double mean_thresh,
                       int dist_thresh_min, double* scaled_out, uint8_t* flag_out,
                       uint8_t* d_flag_out, double* d_scaled_out);

/* The disp pixels of one chromosome on the device (analysis.py:169-183 for
 * estimate_disp, :261-275 for lrt): the union pixels whose d_disp_idx (n,
 * 0/1) is set, in pixel order -> d_raw_out (n_disp, R) int32, d_f_out
 * (n_disp, R) = bias[row] * bias[col] * sf (numpy's products in numpy's
 * order), d_dist_out (n_disp) = col - row. Inputs: d_row / d_col (n),
 * d_raw (n, R) int32, d_sf (n, R), or (R,) with sf_per_rep (the
 * non-conditional norms, broadcast as analysis.py:274-275 does), bias
 * (n_bins, R) on the HOST (core.py:35-60, filtered). n_disp = the caller's
 * count of set flags (H3D_EARG if the device counts another). Synchronous. */
int h3d_disp_pixels_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_col,
                        const int32_t* d_raw, const double* d_sf, int sf_per_rep,
                        const double* bias, int n_bins, const uint8_t* d_disp_idx,
                        int64_t n, int R, int64_t n_disp, int32_t* d_raw_out,
                        double* d_f_out, int32_t* d_dist_out);

/* f of pixels received by the distance re-shard, rebuilt from their keys
 * (replaces shipping f; analysis.py:169-183 forms it on the rank that
 * prepared the chromosome): pixel j of genome chromosome d_chrom[j] at
 * (d_row[j], d_row[j] + d_dist[j]) with size-factor row d_sfi[j] gets
 * d_f_out[j, k] = (bias[row, k] * bias[col, k]) * sf[sfi, k] -- the product
 * and order of h3d_disp_pixels_dev, so bit for bit the sender's f. d_bias
 * (B, R): every chromosome's (filtered) bias rows stacked, chromosome g's
 * from d_boff[g] (nchrom + 1 offsets); d_sf (S, R) its size-factor rows from
 * d_soff[g]. A key outside its chromosome's rows is H3D_EINPUT (its f NaN).
 * Synchronous. */
int h3d_pixel_f_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_dist,
                    const int32_t* d_chrom, const int32_t* d_sfi, int64_t n, int R,
                    const double* d_bias, const int64_t* d_boff, const double* d_sf,
                    const int64_t* d_soff, int nchrom, double* d_f_out);

/* ---- estimate_disp ----------------------------------------------------- */

/* Per-(distance, condition) dispersion (analysis.py:185-206). raw/f (n, R),
 * dist (n) in [0, D); cond_of_rep (R) in [0, C). Output disp_per_dist (D, C)
 * (NaN for empty slices), seg_flags (D, C) optional. */
int h3d_disp_per_dist(h3d_ctx* ctx, const int64_t* raw, const double* f,
                      const int32_t* dist, int64_t n, int R, int C,
                      const int32_t* cond_of_rep, int D, int estimator,
                      double* disp_per_dist, int32_t* seg_flags);

/* Same on device-resident inputs: d_raw (n, R) int32, d_f (n, R), d_dist (n).
 * `reduce` (optional) makes the per-segment sums global across ranks; every
 * rank must pass the same D, C, cond_of_rep. */
int h3d_disp_per_dist_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                          const int32_t* d_dist, int64_t n, int R, int C,
                          const int32_t* cond_of_rep, int D, int estimator,
                          double* disp_per_dist, int32_t* seg_flags,
                          h3d_allreduce_fn reduce, void* user);

/* Work of the last h3d_disp_per_dist[_dev] / h3d_estimate_disp_dev call on
 * the ctx, per (distance, condition) segment s = d * C + c (S = D * C):
 * qcml iterations (equalize passes) and bounded-Brent NLL evaluations. The
 * multi-GPU distance owners balance on these (measurement). */
int h3d_disp_seg_stats(h3d_ctx* ctx, int S, int32_t* qiter, int32_t* evals);

/* Smoothed dispersion function of one condition, tabulated at d = 0..D-1
 * (lowess.py:95-244 weighted_lowess_fit if weighted, else lowess_fit;
 * left_boundary = first finite value, as analysis.py:212). frac < 0 = auto.
 * weighted: 0 lowess_fit; 1 weighted, the smallest scaled weight pinned to
 * exactly 1; 2 weighted with the reference's own
 * w * (1 / w) scaling (lowess.py:183-184), whose floor (:201) drops a
 * minimum weight that rounds to 1 - 2^-53. Every weighted entry point below
 * takes the same three values. */
int h3d_disp_table(const double* disp_per_dist_col, int D, int weighted,
                   double frac, double auto_frac_factor, double* table_out);

/* h3d_disp_table for every column of disp_per_dist (D, C), row-major in and
 * out, the conditions on concurrent host threads (analysis.py:208-219's
 * per-condition loop). */
int h3d_disp_tables(const double* disp_per_dist, int D, int C, int weighted,
                    double frac, double auto_frac_factor, double* tables_out);

/* The same tables computed on the GPU (one workgroup per condition, D <=
 * 1024; larger D runs the host smoother inside the call), device buffers
 * in and out, enqueued on the ctx stream without waiting: the estimate_disp
 * -> lrt step stays on the device (analysis.py:226-240 between :198-246 and
 * :249-276). Its status is settled by the next h3d_lrt_dev_tab (which
 * re-runs the LRT if a degenerate fit had to be redone on the host) or by
 * h3d_disp_tables_wait; both return the reference's error as
 * h3d_disp_tables would. The buffers must stay valid until then. */
int h3d_disp_tables_dev(h3d_ctx* ctx, const double* d_disp_per_dist, int D,
                        int C, int weighted, double frac,
                        double auto_frac_factor, double* d_tables_out);
int h3d_disp_tables_wait(h3d_ctx* ctx);

/* estimate_disp (qcml, h3d_disp_per_dist_dev without a reduce) whose
 * smoothed tables are computed on the device from the result in place
 * (analysis.py:198-246 then :226-240): disp_per_dist (D, C) on the host as
 * h3d_disp_per_dist_dev returns it, the tables into d_tables_out (device,
 * (D, C)), the smoother running while the call returns. Settled like
 * h3d_disp_tables_dev; it reads the ctx's result buffer, so the next
 * estimate_disp call on the ctx must come after h3d_lrt_dev_tab /
 * h3d_disp_tables_wait. */
int h3d_estimate_disp_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                          const int32_t* d_dist, int64_t n, int R, int C,
                          const int32_t* cond_of_rep, int D, int weighted,
                          double frac, double auto_frac_factor,
                          double* disp_per_dist, int32_t* seg_flags,
                          double* d_tables_out);

/* disp[i, c] = tables[dist[i], c] on the device (analysis.py:218 disp_fn(dist)
 * at integer distances = the tabulation; NaN outside [0, D)): d_tables (D,
 * C), d_dist (n) -> d_disp_out (n, C). A pending h3d_disp_tables_dev /
 * h3d_estimate_disp_dev table is settled first (h3d_disp_tables_wait).
 * Synchronous. */
int h3d_table_gather_dev(h3d_ctx* ctx, const double* d_tables, int D, int C,
                         const int32_t* d_dist, int64_t n, double* d_disp_out);

/* ---- lrt --------------------------------------------------------------- */

/* Per-pixel LRT (lrt.py:7-50) with disp[i, c] = disp_table[dist[i], c]
 * (disp_table (D, C)); with dist == NULL, disp_table is the per-pixel
 * dispersion array (n, C) itself (the reference's disp_<chrom>.npy, as
 * analysis.py:269-278 loads it). Outputs p, llr, mu0 (n), mu1 (n, C);
 * disp_out (n, C) optional. */
int h3d_lrt(h3d_ctx* ctx, const int64_t* raw, const double* f,
            const int32_t* dist, const double* disp_table, int64_t n, int R,
            int C, const int32_t* cond_of_rep, int D, int refit_mu, double* p,
            double* llr, double* mu0, double* mu1, double* disp_out);

int h3d_lrt_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                const int32_t* d_dist, const double* disp_table, int64_t n,
                int R, int C, const int32_t* cond_of_rep, int D, int refit_mu,
                double* d_p, double* d_llr, double* d_mu0, double* d_mu1,
                double* d_disp);

/* h3d_lrt_dev with the per-distance table (D, C) in DEVICE memory (from
 * h3d_disp_tables_dev; d_dist required). */
int h3d_lrt_dev_tab(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                    const int32_t* d_dist, const double* d_disp_table,
                    int64_t n, int R, int C, const int32_t* cond_of_rep, int D,
                    int refit_mu, double* d_p, double* d_llr, double* d_mu0,
                    double* d_mu1, double* d_disp);

/* lrt.py:7-50 with the reference's own disp argument: per pixel AND
 * replicate dispersions disp_wide (n, R) (lrt.py's `disp`, as analysis.py:277
 * builds it with np.dot(disp, design.T); any (n, R) values are taken as
 * given). Outputs as h3d_lrt. */
int h3d_lrt_wide(h3d_ctx* ctx, const int64_t* raw, const double* f,
                 const double* disp_wide, int64_t n, int R, int C,
                 const int32_t* cond_of_rep, int refit_mu, double* p,
                 double* llr, double* mu0, double* mu1);

/* dispersion.py:46-80 cml on given data (n, r), already divided by f: the
 * bounded-Brent minimisation of the NB conditional NLL on the GPU (one
 * k_brent search); *disp = delta / (1 - delta). H3D_ENOCONV where the
 * reference's assert res.success would fail. */
int h3d_cml(h3d_ctx* ctx, const double* data, int64_t n, int r, double* disp);

/* ---- scaled NB operators (util/scaled_nb.py) ---------------------------- */

/* The functions dispersion.qcml and lrt.lrt import (dispersion.py:5,
 * lrt.py:4), one lane per pixel in the caller's pixel order, replicate-minor
 * (n, R) rows, 1 <= R <= 32 (H3D_EINPUT otherwise). A pixel's failure does
 * not fail the call: the H3D_FLAG_* bits of every pixel are OR-ed into
 * *flags (may be NULL), the return code stays 0, and that pixel's outputs are
 * NaN -- the caller raises what the reference raises. Host entries upload,
 * launch and download (counts int64, H3D_EINPUT outside [0, 2^31)); the _dev
 * entries take device pointers (counts int32) on the ctx's stream and wait
 * for it only to read the flags. n = 0 launches nothing. */

/* scaled_nb.py:71-183 fit_mu_hat: mu (n) = the MLE of the mean under fixed
 * dispersions. alpha is read at alpha[i * alpha_px_stride + k *
 * alpha_rep_stride] and holds only the values so addressed: the reference's
 * broadcast forms (:110-127) scalar (0, 0), (R,) (0, 1), (n, 1) (1, 0) and
 * (n, R) (R, 1); other strides are H3D_EARG. H3D_FLAG_BADIN: the asserts of
 * :139-141; H3D_FLAG_NOROOT: an all-zero row (the brentq fallback's
 * ValueError, :172-181); H3D_FLAG_NOCONV: the solver's step limit. */
int h3d_nb_fit_mu(h3d_ctx* ctx, const int64_t* x, const double* b,
                  const double* alpha, int64_t alpha_px_stride,
                  int64_t alpha_rep_stride, int64_t n, int R, double* mu,
                  int* flags);
int h3d_nb_fit_mu_dev(h3d_ctx* ctx, const int32_t* d_x, const double* d_b,
                      const double* d_alpha, int64_t alpha_px_stride,
                      int64_t alpha_rep_stride, int64_t n, int R, double* d_mu,
                      int* flags);

/* scaled_nb.py:186-214 equalize: pseudo (n, R) from counts x and factors f at
 * the dispersion alpha, or at alpha_px[i] per pixel when alpha_px is not NULL
 * (the reference's code takes that form too: q2qnbinom's alpha is "one per
 * x", :230-232). The clamp of mu_out at 0.25 carries from one replicate into
 * the next as the reference's in-place update does (:209-213, :240-242).
 * mu_hat (n), optional: the fitted means (:208). Flags as h3d_nb_fit_mu. */
int h3d_nb_equalize(h3d_ctx* ctx, const int64_t* x, const double* f,
                    double alpha, const double* alpha_px, int64_t n, int R,
                    double* pseudo, double* mu_hat, int* flags);
int h3d_nb_equalize_dev(h3d_ctx* ctx, const int32_t* d_x, const double* d_f,
                        double alpha, const double* d_alpha_px, int64_t n,
                        int R, double* d_pseudo, double* d_mu_hat, int* flags);

/* scaled_nb.py:217-275 q2qnbinom, elementwise over n values: out[i] = x[i]
 * carried from NB(mu_in[i]) to NB(mu_out[i]) at the dispersion alpha, or
 * alpha_el[i] when alpha_el is not NULL. mu_in / mu_out are read AND
 * written: where either is below 0.25 both come back as 0.25, as the
 * reference mutates its arguments (:240-242). */
int h3d_nb_quantile_map(h3d_ctx* ctx, const double* x, double* mu_in,
                        double* mu_out, double alpha, const double* alpha_el,
                        int64_t n, double* out);

/* scaled_nb.py:12-33 logpmf, elementwise over n values of k, m, phi. */
int h3d_nb_logpmf(h3d_ctx* ctx, const double* k, const double* m,
                  const double* phi, int64_t n, double* out);

/* ---- negative-binomial sampling (simulate on the GPU) -------------------- */

/* The draws of util/simulation.py:84-99 (reference simulation.py:187-203:
 * one np.random.negative_binomial array per replicate) from a counter-based
 * stream instead of numpy's sequential one. The draw of a pixel is a pure
 * function of (seed, stream, rep, pixel index): Philox4x32-10 with key =
 * (seed low word, seed high word) and counter = {index low word, index high
 * word, rep, stream} gives four words w0..w3; u1 = ((w1:w0 >> 12) + 1/2)
 * 2^-52 and u2 the same of w3:w2; the Poisson mean is lambda = bm disp
 * gammaincinv(1 / disp, u1) (bm disp gammainccinv(1 / disp, 1 - u1) above
 * 1/2) and the count the smallest k with pdtr(k, lambda) >= u2 (DESIGN.md §1
 * F9). The pixel index of element i is pixel0 + i, so a slice of a pixel list
 * drawn with its offset equals the slice of the whole list's draws. bm or
 * disp not positive finite, or lambda not below 2^31: count -1 and
 * H3D_FLAG_BADIN in *flags (may be NULL); the return code stays 0. */

/* simulation.py:187-203 for one replicate whose biased means bm (n) and
 * dispersions disp (n) the caller formed: counts (n) int32 and, when lambda
 * is not NULL, the gamma stage's lambda (n). */
int h3d_nb_sample(h3d_ctx* ctx, const double* bm, const double* disp, int64_t n,
                  uint64_t seed, uint32_t stream, uint32_t rep, int64_t pixel0,
                  int32_t* counts, double* lambda, int* flags);
int h3d_nb_sample_dev(h3d_ctx* ctx, const double* d_bm, const double* d_disp,
                      int64_t n, uint64_t seed, uint32_t stream, uint32_t rep,
                      int64_t pixel0, int32_t* d_counts, double* d_lambda,
                      int* flags);

/* simulation.py:187-203 for all J replicates (1 <= J <= 32) of one
 * chromosome, fused: replicate j takes meanA (j < J / 2) or meanB, bm = mean
 * x (bias[row, j] x bias[col, j] x sf) with bias (n_bins, J) and sf =
 * d_sf[j] (sf_rows = 1) or d_sf[dist x J + j] (sf_rows = D), dist = col - row,
 * disp = d_table[dist] (D entries), rep = j. d_counts: (J, n) int32, one
 * contiguous plane per replicate. A pixel with row or col outside [0, n_bins)
 * or dist outside [0, D) gets -1 and H3D_FLAG_BADIN. */
int h3d_simulate_dev(h3d_ctx* ctx, const int32_t* d_row, const int32_t* d_col,
                     const double* d_meanA, const double* d_meanB,
                     const double* d_bias, const double* d_sf, int sf_rows,
                     const double* d_table, int D, int64_t n, int J, int n_bins,
                     uint64_t seed, uint32_t stream, int64_t pixel0,
                     int32_t* d_counts, int* flags);

/* ---- bh ---------------------------------------------------------------- */

/* Benjamini-Hochberg q-values over the finite p-values (NaN elsewhere), on
 * the host CPU (no ctx). */
int h3d_bh(const double* p, int64_t n, double* q);

/* The same on the ctx's GPU: one radix sort of (p, index), the ratio
 * p_(j) / ((j + 1) / m), a reverse min-scan, a scatter -- bit-identical to
 * h3d_bh. _ctx: host buffers (synchronous); _dev: device buffers, stream-
 * ordered on the ctx stream (n < 2^31). */
int h3d_bh_ctx(h3d_ctx* ctx, const double* p, int64_t n, double* q);
int h3d_bh_dev(h3d_ctx* ctx, const double* d_p, int64_t n, double* d_q);

/* The same BH over p-values sharded across ranks (analysis.py:286-303 over
 * every chromosome, hic3defdr_amd.parallel.bh_sharded; the rank exchange is
 * the caller's). Device buffers on the ctx stream, each call returns once
 * the stream has drained (the caller moves the results between ranks next);
 * every q has h3d_bh_dev's bits.
 *   _sort: (p, val) pairs sorted by p ascending, non-finite p last (key
 *     +inf); val NULL = 0..n-1; *m_finite (host, synchronous) = finite count.
 *   _scan: for a bucket of mb sorted finite p-values at global ranks
 *     offset .. offset + mb - 1 of m: scanned[j] = min over j' >= j of
 *     p[j'] / ((offset + j' + 1) / m); *bucket_min (host, synchronous) =
 *     scanned[0] (+inf for an empty bucket).
 *   _finish: q[j] = min(scanned[j], higher_min) clipped at 1, higher_min =
 *     the minimum of the higher buckets' bucket_min (+inf for the last). */
int h3d_bh_sort_dev(h3d_ctx* ctx, const double* d_p, const int64_t* d_val, int64_t n,
                    double* d_key_out, int64_t* d_val_out, int64_t* m_finite);
int h3d_bh_scan_dev(h3d_ctx* ctx, const double* d_ps, int64_t mb, int64_t offset,
                    int64_t m, double* d_scanned, double* bucket_min);
int h3d_bh_finish_dev(h3d_ctx* ctx, const double* d_scanned, int64_t mb, double higher_min,
                      double* d_q);

/* ---- threshold / classify / collect (host) ------------------------------ */

/* Clusters of a pixel list (clusters.py:73-97 find_clusters with its
 * DirectedDisjointSet, :15-70): connectivity 1 = 4-neighbour cross, 2 = the
 * 8-neighbourhood (scipy generate_binary_structure(2, connectivity)).
 * label[i] = cluster of pixel i, numbered in the order of the reference's
 * get_groups() list; *n_clusters = number of clusters. Host code. */
int h3d_find_clusters(const int64_t* row, const int64_t* col, int64_t n,
                      int connectivity, int64_t* label, int64_t* n_clusters);

/* h3d_find_clusters plus the pixel order the reference writes: order (n) =
 * the pixel indices cluster by cluster (get_groups() order), each cluster in
 * the iteration order of the reference's Python set of (i, j) tuples --
 * CPython 3.8-3.10's set table replayed over the same adds and |= merges
 * (clusters.py:34-66), which is the order save_clusters (clusters.py:129-130)
 * and clusters_to_table (cluster_table.py:64-78, list(cluster)) write.
 * The pixels must be distinct. Host code. */
int h3d_find_clusters_ordered(const int64_t* row, const int64_t* col, int64_t n,
                              int connectivity, int64_t* label, int64_t* n_clusters,
                              int64_t* order);

/* "[[i, j], [i, j], ...]" text of each cluster (clusters.py:129-130 JSON,
 * cluster_table.py:67 TSV "cluster" column): cluster k is the pixels
 * order[starts[k] .. starts[k+1]). Concatenated into buf (cap bytes; NULL to
 * size), ends[k] = end offset of cluster k (optional), *len = total bytes. */
int h3d_format_clusters(const int64_t* row, const int64_t* col,
                        const int64_t* order, const int64_t* starts,
                        int64_t n_clusters, char* buf, int64_t cap,
                        int64_t* ends, int64_t* len);

/* ---- threshold / classify on the GPU ------------------------------------- */

/* The calls as connected components. The pixels (row[i], col[i]) come in the
 * outdir layout: strictly increasing in (row, col) order (so distinct),
 * coordinates in [0, 2^31), n <= 2^31 - 2; cls (n) is a class byte per pixel,
 * 255 = no pixel. Two pixels connect when they are adjacent (connectivity 1 =
 * an edge, 2 = an edge or a corner) and of equal class, so every class is
 * clustered in the one pass. The partition is that of find_clusters
 * (clusters.py:69-97) per class: its directed bookkeeping orders the output,
 * never the membership. The ORDER is not the reference's but canonical:
 * label[i] (int32; -1 for a class-255 pixel) numbers the clusters by their
 * first pixel in (row, col) order, 0 .. *n_clusters - 1. The input rule is
 * checked once per call on the device; an input that breaks it sets
 * H3D_FLAG_BADIN in *flags beside rc 0 (label all -1, *n_clusters 0).
 * H3D_EARG for a connectivity other than 1 or 2. Labels depend on nothing but
 * the input (run-based union-find with the smallest id as representative;
 * integer atomics only). _dev: row, col, cls and label are device pointers;
 * n_clusters and flags are host words either way. Synchronous. */
int h3d_label_components(h3d_ctx* ctx, const int64_t* row, const int64_t* col,
                         const uint8_t* cls, int64_t n, int connectivity,
                         int32_t* label, int64_t* n_clusters, int* flags);
int h3d_label_components_dev(h3d_ctx* ctx, const int64_t* d_row,
                             const int64_t* d_col, const uint8_t* d_cls,
                             int64_t n, int connectivity, int32_t* d_label,
                             int64_t* n_clusters, int* flags);

/* The class byte of threshold (thresholding.py:7-41): d_cls[i] = 0 where
 * d_q[i] < fdr (sig), 1 where d_q[i] >= fdr (insig), 255 for a NaN (in
 * neither). Device pointers; synchronous. */
int h3d_threshold_classes_dev(h3d_ctx* ctx, const double* d_q, int64_t n,
                              double fdr, uint8_t* d_cls);

/* The class byte of classify (classification.py:7-49): for a pixel with
 * d_member[i] != 0, np.argmax of its row of d_value (n, C) row-major -- the
 * first maximum, and the first NaN wins; 255 for the others. 1 <= C <= 254
 * (H3D_EARG otherwise). Device pointers; synchronous. */
int h3d_argmax_classes_dev(h3d_ctx* ctx, const double* d_value, int64_t n,
                           int C, const uint8_t* d_member, uint8_t* d_cls);

/* The clusters of h3d_label_components as lists (the arrays of
 * thresholding.py:7-41 / classification.py:7-49's results): per cluster k of
 * n_clusters its size[k] (int32), cls_of[k] = the class byte of its first
 * member, and bounds (4, n_clusters) int32 = min row, max row, min col, max
 * col. A cluster is kept when size >= max(min_size, 1); the kept clusters, in
 * label order, are members[starts[j] .. starts[j + 1]) -- pixel indices in
 * increasing order, so each cluster is in (row, col) order. All buffers are
 * the caller's: members has room for n entries (*n_members are meaningful; the
 * _dev form uses all n as sort space), starts for n_clusters + 1 (*n_kept + 1
 * are written). A label outside [-1, n_clusters) is H3D_EARG. _dev: every
 * array is a device pointer; n_kept and n_members are host words either way.
 * Synchronous. */
int h3d_cluster_lists(h3d_ctx* ctx, const int32_t* label, const uint8_t* cls,
                      const int64_t* row, const int64_t* col, int64_t n,
                      int64_t n_clusters, int64_t min_size, int32_t* size,
                      uint8_t* cls_of, int32_t* bounds, int32_t* members,
                      int64_t* starts, int64_t* n_kept, int64_t* n_members);
int h3d_cluster_lists_dev(h3d_ctx* ctx, const int32_t* d_label,
                          const uint8_t* d_cls, const int64_t* d_row,
                          const int64_t* d_col, int64_t n, int64_t n_clusters,
                          int64_t min_size, int32_t* d_size, uint8_t* d_cls_of,
                          int32_t* d_bounds, int32_t* d_members,
                          int64_t* d_starts, int64_t* n_kept,
                          int64_t* n_members);

/* Per-cluster statistics of a sparse table (cluster_table.py:192-332
 * add_columns_to_cluster_table's arithmetic). The table is n pixels (row[i],
 * col[i]) int64 with coordinates in [0, 2^31), n <= 2^31 - 2, in any order,
 * and data (n, K) float64 row-major, 1 <= K <= 256. sorted != 0 promises the
 * outdir layout -- strictly increasing (row, col) -- which is verified on the
 * device and saves the sort. Cluster k of n_clusters is the pixels prow / pcol
 * [starts[k] .. starts[k + 1]) in list order (a pixel listed twice counts
 * twice), starts[0] = 0, at most 2^31 - 2 pixels in all. A cluster pixel's
 * value is the table's at its (row, col), or 0.0 where the table has no such
 * pixel; per cluster and column the m values are reduced to mean (sum / m),
 * max and min (a NaN among the m makes max and min NaN; every NaN is stored as
 * 0x7ff8000000000000). want is a bit set of H3D_CSTAT_MEAN / _MAX / _MIN; each
 * wanted output is (n_clusters, K) float64, the others may be NULL. found
 * (n_clusters) int32, may be NULL: how many of the cluster's pixels the table
 * holds. Bad input sets bits in *flags beside rc 0, and the outputs are then
 * unspecified: H3D_CSTAT_REPEAT a table pixel twice or outside [0, 2^31),
 * H3D_CSTAT_ORDER a broken `sorted` promise, H3D_CSTAT_PIXEL a cluster pixel
 * outside [0, n_rows) x [0, n_cols), H3D_CSTAT_STARTS starts[0] != 0 or a
 * cluster without pixels. n_clusters = 0 launches nothing; n = 0 is legal
 * (every value 0). The sums are stored and folded in a fixed order (no
 * floating-point atomics): a cluster's results depend on its own pixel list,
 * the table and K alone, and repeat bit for bit. _dev: every array is a
 * device pointer; flags is a host word either way. Synchronous. */
#define H3D_CSTAT_MEAN 1
#define H3D_CSTAT_MAX 2
#define H3D_CSTAT_MIN 4
#define H3D_CSTAT_REPEAT 1
#define H3D_CSTAT_ORDER 2
#define H3D_CSTAT_PIXEL 4
#define H3D_CSTAT_STARTS 8
int h3d_cluster_stats(h3d_ctx* ctx, const int64_t* row, const int64_t* col,
                      const double* data, int64_t n, int K, int sorted,
                      int64_t n_rows, int64_t n_cols, const int64_t* prow,
                      const int64_t* pcol, const int64_t* starts,
                      int64_t n_clusters, int want, double* mean, double* vmax,
                      double* vmin, int32_t* found, int* flags);
int h3d_cluster_stats_dev(h3d_ctx* ctx, const int64_t* d_row,
                          const int64_t* d_col, const double* d_data,
                          int64_t n, int K, int sorted, int64_t n_rows,
                          int64_t n_cols, const int64_t* d_prow,
                          const int64_t* d_pcol, const int64_t* d_starts,
                          int64_t n_clusters, int want, double* d_mean,
                          double* d_max, double* d_min, int32_t* d_found,
                          int* flags);

/* ---- alternative models (analysis/alternatives.py) ---------------------- */

/* Poisson LRT (alternatives.py:25-42 with refit_mu=True, the only mode
 * Poisson3DeFDR uses and the only one the reference can run: its refit_mu=False
 * branch builds mu_hat_alt transposed and fails in np.dot). mu0 =
 * np.average(raw / f, weights=f) over all replicates, mu1[:, c] the same over
 * condition c's; llr = sum log poisson.pmf(raw | mu0 f) - sum log
 * poisson.pmf(raw | mu1[cond] f); p = chi2(C - 1).sf(-2 llr). raw/f (n, R) ->
 * p, llr, mu0 (n), mu1 (n, C). */
int h3d_lrt_poisson(h3d_ctx* ctx, const int64_t* raw, const double* f,
                    int64_t n, int R, int C, const int32_t* cond_of_rep,
                    double* p, double* llr, double* mu0, double* mu1);
int h3d_lrt_poisson_dev(h3d_ctx* ctx, const int32_t* d_raw, const double* d_f,
                        int64_t n, int R, int C, const int32_t* cond_of_rep,
                        double* d_p, double* d_llr, double* d_mu0,
                        double* d_mu1);

/* Per-pixel method-of-moments dispersion of every condition's replicates
 * (dispersion.py:83-104 mme_per_pixel(data[:, design[:, c]], f)): data (n, R)
 * (divided by f (n, R) when f != NULL) -> disp (n, C) = max((var - mean) /
 * mean^2, min_disp), var with ddof 1; NaN stays NaN (numpy maximum).
 * min_disp = -inf for no floor; Unsmoothed3DeFDR uses 1e-7. */
int h3d_mme_per_pixel(h3d_ctx* ctx, const double* data, const double* f,
                      int64_t n, int R, int C, const int32_t* cond_of_rep,
                      double min_disp, double* disp);

/* ---- dense views (get_matrix / select_matrix / APA) ---------------------- */

/* W dense h x w windows of a sparse matrix in one launch: replaces the
 * per-window host passes of util/matrices.py:132-160 select_matrix (through
 * analysis/core.py:255-291 get_matrix) and of util/apa.py:6-44 make_apa_stack
 * (one scipy slice and toarray per cluster, :36-43).
 * The matrix is CSR, n_rows x n_cols: indices (nnz) int32 strictly ascending
 * within a row, data (nnz, ld) float64 row-major, and either indptr
 * (n_rows + 1) int64 or -- indptr NULL -- row (nnz) int32, the entries sorted
 * by (row, col) as every outdir table is (the row pointers are then built on
 * the device, one search per row). cols (K, host memory in both entry points)
 * lists the data columns taken, each below ld. origins (W, 2) int32 = every
 * window's (row0, col0); out is (K, W, h, w) float64, or with mean != 0
 * (W, h, w): the K columns summed in list order, divided by K
 * (core.py:279-286's np.mean over a condition's replicates).
 * Cell (r, c) of a window is A[row0 + r, col0 + c] when stored, else `fill`;
 * with symmetrize != 0 it is A[col0 + c, row0 + r] when that is stored, else
 * A[row0 + r, col0 + c], else `fill` (select_matrix's second, transposed pass
 * writes last, matrices.py:156-159). Positions outside the matrix are absent,
 * so a window may lie partly or wholly outside it. A window whose row0 is
 * INT32_MIN is all NaN whatever `fill` is (apa.py:38-40). Stored values pass
 * through bit for bit.
 * H3D_EARG: h < 1, w < 1, K < 1 (or above 64), a column not below ld,
 * K * W * h * w >= 2^31, an indptr (host entry) that decreases or leaves
 * [0, nnz]. W = 0 and nnz = 0 succeed. _dev: every array but cols is a device
 * pointer; the gather runs on the ctx stream (the inputs must be complete
 * there) and the call returns once it has finished, like the host entry. */
int h3d_window_gather(h3d_ctx* ctx, const int64_t* indptr, const int32_t* row,
                      const int32_t* indices, const double* data, int64_t nnz,
                      int ld, int n_rows, int n_cols, const int32_t* cols, int K,
                      const int32_t* origins, int64_t W, int h, int w,
                      int symmetrize, int mean, double fill, double* out);
int h3d_window_gather_dev(h3d_ctx* ctx, const int64_t* d_indptr,
                          const int32_t* d_row, const int32_t* d_indices,
                          const double* d_data, int64_t nnz, int ld, int n_rows,
                          int n_cols, const int32_t* cols, int K,
                          const int32_t* d_origins, int64_t W, int h, int w,
                          int symmetrize, int mean, double fill, double* d_out);

/* Per-cell aggregate of a stack (W, h, w) of windows (the np.nanmean(stack,
 * axis=0) that follows util/apa.py:6-44 in an aggregate peak analysis):
 * count (h, w) int64 = the windows whose cell is not NaN, sum (h, w) = their
 * sum, in a fixed order (windows in chunks of 128, each chunk summed window
 * by window, the chunk sums added in chunk order), so a rerun gives the same
 * bits. Host buffers. W = 0 gives zeros. */
int h3d_stack_aggregate(h3d_ctx* ctx, const double* stack, int64_t W, int h,
                        int w, int64_t* count, double* sum);

/* ---- sparse-bin filter and KR balancing (simulation workflow) ------------- */

/* util/filtering.py:8-33 filter_sparse_rows_count on a square CSR matrix
 * (indptr (n + 1) int64, indices (nnz) int32, data (nnz) float64; host
 * buffers, duplicates summed): down[i] / up[j] count the entries with
 * 1 <= col - row <= min(n, k) and data > 0 per row / per column; a bin with
 * up < min_nnz and down < min_nnz is wiped, and an entry whose row or column
 * is wiped leaves, as does a stored 0 (the reference's sparse products drop
 * it). The kept entries come back in their order: out_indptr (n + 1),
 * out_indices / out_data (capacity nnz), *nnz_out their count; *n_wiped
 * (nullable) the wiped bins. min_nnz == 0 or k == 0: nothing leaves
 * (filtering.py:16-17). H3D_EARG: indptr not ascending from 0 to nnz,
 * nnz >= 2^30; H3D_EINPUT: a column outside [0, n). */
int h3d_filter_sparse_rows(h3d_ctx* ctx, const int64_t* indptr,
                           const int32_t* indices, const double* data, int n,
                           int64_t nnz, int min_nnz, int k, int64_t* out_indptr,
                           int32_t* out_indices, double* out_data,
                           int64_t* nnz_out, int64_t* n_wiped);

/* The filter above (skipped when min_nnz == 0 or k == 0) followed by
 * util/balancing.py:5-208 kr_balance in one device pass: the README's loop
 * over the simulated replicates (README.md:602-614). The matrix is upper
 * triangular, canonical CSR (columns ascending from the row's own, no
 * duplicates; host buffers as above); an entry of value 0 is no entry. The
 * device builds the symmetric matrix of the kept entries (rows in ascending
 * column order, the diagonal once) and runs the Knight-Ruiz iteration on the
 * rows that have entries: Newton steps on x (A x) = 1 until
 * |1 - x (A x)|^2 <= tol^2 or more than max_iter steps (max_iter < 0: no
 * cap), each a conjugate-gradient solve clamped to the box [lo, hi]
 * (kr_balance's delta / ddelta); x0 (nullable, n values, those of rows
 * without entries ignored) is the start vector, default ones. Then
 * scale = x sqrt(sum(A) / sum(diag(x) A diag(x))), bias_out (n) = 1 / scale,
 * 0 for the rows without entries -- all NaN when no row has entries, as the
 * reference's 0 * sqrt(0 / 0). balanced_out (nullable, nnz): a_ij s_i s_j of
 * every input entry (0 for the entries that left).
 * stats (6) = {outer steps, inner steps in total, low-clamp hits, high-clamp
 * hits, bins wiped by the filter, rows in the iteration}; hist_inner /
 * hist_norm (nullable, capacity hist_cap): inner steps and |1 - x (A x)|
 * of the first hist_cap outer steps (the reference's "it in. it res" table).
 * Every sum has a fixed order: a rerun gives the same bits.
 * H3D_ENOCONV: more than 10,000 inner steps in total (the reference's inner
 * loop has no cap), or a clamp without a candidate step (the reference
 * raises); H3D_EINPUT: a column outside [row, n); H3D_EARG: negative or NaN
 * tol, indptr not ascending from 0 to nnz, nnz >= 2^30. */
int h3d_kr_balance(h3d_ctx* ctx, const int64_t* indptr, const int32_t* indices,
                   const double* data, int n, int64_t nnz, int min_nnz, int k,
                   double tol, double lo, double hi, int max_iter,
                   const double* x0, double* bias_out, double* balanced_out,
                   int64_t* stats, int32_t* hist_inner, double* hist_norm,
                   int hist_cap);

/* ---- diagnostics: the numbers under the reference's plot_* methods -------- */

/* Every floating-point sum below has one fixed association (lane-strided
 * running sums, an LDS tree, per-block partials, a final pass): a rerun,
 * another launch grid and another ctx give the same bits. No floating-point
 * atomics; counts are integer atomics. n < 2^31 throughout. */

/* sums (K, C) and counts (K) int64 of the rows of values (n, C) row-major
 * grouped by keys (n) int32: a key outside [0, K) drops its row. The members
 * of a key are added in their original order (a stable sort of (key, index),
 * then 16 interleaved slices per key). A key without rows gives 0; a NaN or
 * an infinity stays in its own (key, column) cell. Replaces the per-bin
 * boolean masks of plotting/distance_dependence.py:38-43 and
 * plotting/dispersion.py:138, :182. K <= 4096, C <= 64. _dev: every array is
 * a device pointer; synchronous. */
int h3d_group_sums(h3d_ctx* ctx, const int32_t* keys, const double* values,
                   int64_t n, int K, int C, double* sums, int64_t* counts);
int h3d_group_sums_dev(h3d_ctx* ctx, const int32_t* d_keys,
                       const double* d_values, int64_t n, int K, int C,
                       double* d_sums, int64_t* d_counts);

/* np.histogram(values, bins=edges): counts (E - 1) int64, bin i =
 * [e_i, e_i+1), the last bin closed on the right, NaN and values outside
 * [e_0, e_E-1] dropped. The bin is found by comparing against the edges
 * themselves (binary search), so a value equal to an edge lands where numpy
 * puts it. edges (E <= 4097) finite and strictly increasing, on the host in
 * both forms; _dev: values and counts are device pointers. */
int h3d_histogram(h3d_ctx* ctx, const double* values, int64_t n,
                  const double* edges, int E, int64_t* counts);
int h3d_histogram_dev(h3d_ctx* ctx, const double* d_values, int64_t n,
                      const double* edges, int E, int64_t* d_counts);

/* The MA plot's numbers for scaled (n, R): mean (n, 2) = the sum over the
 * replicates of conditions cond0 / cond1 (design order) over their count
 * (analysis/plotting.py:307), m = log2(mean0) - log2(mean1), a =
 * 0.5 (log2(mean0) + log2(mean1)) (plotting/ma.py:71-72), and label (n) int8:
 * 0 a non-loop pixel, 1 a loop pixel with !(q < fdr) (a NaN q too), 2
 * significant and m > 0, 3 significant and m < 0, -1 significant with m == 0
 * or NaN -- the pixels the reference draws in no series (ma.py:146-155).
 * loop_idx (n) bytes, or NULL: every pixel is a loop pixel. qvalues (n_q): one
 * per loop pixel in order; the pixel -> q-value index is the exclusive scan
 * of loop_idx, done on the device. H3D_EARG: n_q differs from the loop
 * pixels, a condition outside [0, C). Host buffers. */
int h3d_ma_stats(h3d_ctx* ctx, const double* scaled, int64_t n, int R, int C,
                 const int32_t* cond_of_rep, int cond0, int cond1,
                 const uint8_t* loop_idx, const double* qvalues, int64_t n_q,
                 double fdr, double* mean, double* m, double* a,
                 int8_t* label);

/* counts (L, Ex - 1, Ey - 1) int64: np.histogram2d(x, y, bins=[xedges,
 * yedges])[0] of the points of each class label (n) int8 in [0, L); a row
 * with another label, a NaN or an infinite coordinate is dropped. Each axis
 * has h3d_histogram's edge rules. L <= 127, L (Ex - 1) (Ey - 1) < 2^28. Host
 * buffers. */
int h3d_density_grid(h3d_ctx* ctx, const double* x, const double* y,
                     const int8_t* label, int64_t n, int L,
                     const double* xedges, int Ex, const double* yedges,
                     int Ey, int64_t* counts);

/* scipy.stats.rankdata(method='average') of each of the R columns of n
 * (values[c * n + i]): ranks, 1-based, ties share the mean of their ranks;
 * -0.0 and +0.0 are one value. nan_flags (R): 1 where the column holds a NaN;
 * its ranks are all NaN. R <= 32. Host buffers. */
int h3d_rank_average(h3d_ctx* ctx, const double* values, int64_t n, int R,
                     double* ranks, int32_t* nan_flags);

/* corr (R, R): the Pearson correlation of every pair of the R columns of n,
 * centred (column means, sums of products of deviations, s_ij /
 * sqrt(s_ii s_jj), clipped to [-1, 1]; exactly symmetric). ranked != 0: of
 * the columns' average ranks instead (Spearman). A column with a NaN and a
 * constant column give NaN in their row and column, as scipy.stats.pearsonr
 * / spearmanr do. R <= 32. Host buffers. */
int h3d_corr_matrix(h3d_ctx* ctx, const double* values, int64_t n, int R,
                    int ranked, double* corr);

/* mean (n) and var (n) over the n_reps replicates reps[] of scaled (n, R):
 * np.mean(x, axis=1) and np.var(x, ddof=1, axis=1) in numpy's two passes and
 * its row-sum association (analysis/plotting.py:128-129); one replicate
 * gives var = NaN (0 / 0). Host buffers. */
int h3d_pixel_moments(h3d_ctx* ctx, const double* scaled, int64_t n, int R,
                      const int32_t* reps, int n_reps, double* mean,
                      double* var);

/* balanced (n, R) = raw[i, r] / (bias[row[i], r] * bias[col[i], r])
 * (analysis/plotting.py:46-48): a zero bias gives inf or NaN as numpy's
 * division does. raw (n, R) int64, bias (n_bins, R); a row or col outside
 * [0, n_bins) gives NaN. Host buffers. */
int h3d_balance_pixels(h3d_ctx* ctx, const int32_t* row, const int32_t* col,
                       const int64_t* raw, const double* bias, int64_t n,
                       int R, int n_bins, double* balanced);

/* ---- evaluation against simulated truth ---------------------------------- */

/* Every output below is an integer count or the correctly rounded quotient
 * of two counts: the results equal the host code's bit for bit, whatever the
 * launch grid. No floating-point atomics. n < 2^31 throughout. */

/* out (n) bytes: 1 where the query pixel (row[i], col[i]) is in the pixel set
 * {(prow[j], pcol[j])}, k pixels, repeats allowed -- the Python set lookup of
 * analysis.py:117-125 and evaluation.py:38-41. The set's keys row << 32 | col
 * are radix-sorted once on the device, then one binary search per query; the
 * queries may come in any order. A set pixel with a coordinate outside
 * [0, 2^31) is dropped (it can match nothing); a query pixel outside that
 * range is H3D_EARG. k = 0 or n = 0: zeros, no launch. _dev: every array is
 * a device pointer; synchronous. */
int h3d_pixel_membership(h3d_ctx* ctx, const int64_t* row, const int64_t* col,
                         int64_t n, const int64_t* prow, const int64_t* pcol,
                         int64_t k, uint8_t* out);
int h3d_pixel_membership_dev(h3d_ctx* ctx, const int64_t* d_row,
                             const int64_t* d_col, int64_t n,
                             const int64_t* d_prow, const int64_t* d_pcol,
                             int64_t k, uint8_t* d_out);

/* evaluation.py:73-78: scikit-learn's _binary_clf_curve and roc_curve on
 * labels (n) bytes (non-zero = positive) and scores (n), plus the FDR points,
 * from one radix sort of (score, label). complement != 0: the score is
 * 1 - scores[i], formed on the device (evaluate() passes q-values). Per run
 * of equal scores (-0.0 and +0.0 one value), descending: tps = the positives
 * so far, fps = the rest, thresh = the score; with drop_intermediate and more
 * than two runs, only the first, the last and those where the second
 * difference of fps or of tps is non-zero; then the origin (0, 0,
 * thresh[1] + 1) in front (scikit-learn 0.24's opening). fpr = fps /
 * fps[m - 1], tpr = tps / tps[m - 1] (0 / 0 = NaN, as the host's); fdr[i] =
 * fps[i] / (fps[i] + tps[i]) at i = start, start + rate, ..., NaN elsewhere,
 * rate = max(m / n_fdr_points, 1), start = the first i with tps[i] > 0 (0
 * without one). The six outputs have room for n + 1 entries; *m_out = the
 * number of points m written to each. *flags: H3D_FLAG_BADIN when a score is
 * NaN (scikit-learn raises; the outputs are then meaningless). n >= 1,
 * n_fdr_points >= 1. _dev: labels, scores and the six outputs are device
 * pointers; synchronous. */
int h3d_roc_curve(h3d_ctx* ctx, const uint8_t* labels, const double* scores,
                  int64_t n, int64_t n_fdr_points, int drop_intermediate,
                  int complement, double* fdr, double* fpr, double* tpr,
                  double* thresh, int64_t* fps, int64_t* tps, int64_t* m_out,
                  int* flags);
int h3d_roc_curve_dev(h3d_ctx* ctx, const uint8_t* d_labels,
                      const double* d_scores, int64_t n, int64_t n_fdr_points,
                      int drop_intermediate, int complement, double* d_fdr,
                      double* d_fpr, double* d_tpr, double* d_thresh,
                      int64_t* d_fps, int64_t* d_tps, int64_t* m_out,
                      int* flags);

/* out[j] = the value at rank ranks[j] (0-based, in [0, n)) of values (n)
 * sorted ascending with every NaN last, K <= 64 ranks; *nan_count = the NaNs.
 * The order statistics np.percentile interpolates between
 * (plotting/distance_bias.py:103); the interpolation itself stays on the
 * host. Host buffers. */
int h3d_order_stats(h3d_ctx* ctx, const double* values, int64_t n,
                    const int64_t* ranks, int K, double* out,
                    int64_t* nan_count);

/* plotting/distance_bias.py:106-112 for B <= 64 inclusive distance ranges
 * [lo[b], hi[b]] (they may overlap; an open end is INT64_MIN / INT64_MAX):
 * members[b] = the pixels with dist in the range, below[b] = those of them
 * with p < p_star (a NaN p or p_star counts as not below). Host buffers. */
int h3d_bin_fractions(h3d_ctx* ctx, const double* p, const int64_t* dist,
                      int64_t n, const int64_t* lo, const int64_t* hi, int B,
                      double p_star, int64_t* members, int64_t* below);

/* ---- measurement -------------------------------------------------------- */

/* Per-kernel HIP-event timing on the ctx stream; on = 0 off, 1 the roofline
 * kernels only ("disp_work", "lrt"), 2 every scope. Events are read back
 * lazily (profile_read / profile_reset). name in {"disp_work" (the
 * equalize pass), "disp_nll", "disp_reduce", "disp_update", "disp_prep",
 * "lrt"}. units: algorithmic HBM bytes for "disp_work" / "disp_nll"
 * (counted on the device since the last reset), pixels for "lrt" /
 * "disp_prep"; h3d_kr_balance's stages are "kr_filter", "kr_symmetrise",
 * "kr_iter" (the Newton loop, its record reads included) and "kr_rescale".
 * name "gang_aborts": *launches = gang Brent waits of the ctx
 * that timed out (the searches then finished under k_brent). */
int h3d_profile_enable(h3d_ctx* ctx, int on);
int h3d_profile_read(h3d_ctx* ctx, const char* name, double* total_ms,
                     int64_t* launches, int64_t* units);
int h3d_profile_reset(h3d_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* H3D_H_ */
