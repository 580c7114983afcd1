/* iamx.h -- C ABI of libiamx.so: the MI355X (gfx950) feature-matching and sparse
 * bundle-adjustment hot path of NorthStarUAS/ImageAnalysis.
 *
 * Conventions
 *   - every entry point returns 0 on success, a negative IAMX_E* code otherwise;
 *     iamx_last_error() gives the message of the calling thread's last failure.
 *   - every pointer marked DEV is a HIP device pointer (e.g. torch.Tensor.data_ptr());
 *     HOST pointers are ordinary host memory.  The caller allocates every buffer.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only
 *     enqueue work, the caller synchronises.  No hidden globals, no allocation.
 *   - reference citations are file:line in NorthStarUAS/ImageAnalysis.
 *
 * A reference-side binding (ctypes) is shown in INTEGRATION.md.
 */
#ifndef IAMX_H
#define IAMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IAMX_OK            0
#define IAMX_EINVAL       -1   /* bad argument (null pointer, size out of range)        */
#define IAMX_ELAUNCH      -2   /* HIP reported a launch / runtime error                 */
#define IAMX_ENODEVICE    -3   /* no gfx950 device visible                              */
#define IAMX_EUNSUPPORTED -4   /* valid input of a kind this path does not handle       */
#define IAMX_ENOMEM       -5   /* a host routine could not allocate its work arrays     */

#define IAMX_DESC_DIM      128 /* SIFT descriptor length (scripts/lib/image.py:324)      */
#define IAMX_ROW_PAD       128 /* packed images are padded to a multiple of this many rows */

int         iamx_version(void);
const char *iamx_last_error(void);
/* name of the architecture the kernels were compiled for ("gfx950") */
const char *iamx_arch(void);

/* ------------------------------------------------------------------------------------
 * Descriptor store.  cv2.SIFT hands the reference float32 rows holding integers 0..255
 * (scripts/lib/image.py:324, cache format :204-217).  The device store keeps them as
 * int8 (value-128), each image padded to IAMX_ROW_PAD rows of zeros, plus two int32 per
 * row: norm_q = sum((a-128)^2) and norm_t = norm_q + 2*sum(a-128), so that
 *     sum((a-b)^2) = norm_q[a] + norm_t[b] + 2 * sum((127-a)*(b-128))      (exact, int32)
 * and the inner sum is one i8 MFMA contraction.
 * ------------------------------------------------------------------------------------ */
/* rows of storage needed for an image with n_rows descriptors */
int64_t iamx_desc_padded_rows(int64_t n_rows);

/* src: DEV [n_rows][128] uint8 (or float32 integer-valued for _f32; values are clamped
 * to 0..255 after rounding to nearest).  dst: DEV [padded_rows][128] int8;
 * norm_q/norm_t: DEV [padded_rows] int32. */
int iamx_desc_pack_u8(const uint8_t *src, int64_t n_rows, int8_t *dst,
                      int32_t *norm_q, int32_t *norm_t, void *stream);
int iamx_desc_pack_f32(const float *src, int64_t n_rows, int8_t *dst,
                       int32_t *norm_q, int32_t *norm_t, void *stream);
/* the inverse for n_img images of a packed store: image i's rows (first stored row img_off[i]) as
 * uint8 at rows [dst_off[i], dst_off[i+1]) of dst -- the source a different layout of the same
 * images is packed from once their descriptors have left the host (scripts/lib/matcher.py:1012-1026
 * drops them from memory on a timer).  img_off DEV [n_img] int32, dst_off DEV [n_img+1] int64. */
int iamx_desc_unpack_u8(const int8_t *desc, const int32_t *img_off, const int64_t *dst_off, int n_img,
                        int max_rows_per_image, uint8_t *dst, void *stream);

/* ------------------------------------------------------------------------------------
 * K2: exact 2-nearest-neighbour search in L2 -- replaces
 *   the_matcher.knnMatch(des1, des2, k=2)           scripts/lib/matcher.py:212-214
 * (FLANN there; the exact search FLANN approximates == cv2.BFMatcher(NORM_L2)).
 * For every query row: the two train rows with the smallest squared distance, nearest
 * first, equal distances ordered by train index (lowest first).  cv2's DMatch.distance
 * is float32(sqrt(float32(d2))).
 *
 * Batched form: one launch matches many ordered (query image, train image) pairs out of
 * one packed descriptor store.
 *   desc/norm_q/norm_t  DEV  packed store (all images back to back)
 *   img_off  DEV [n_img] int32  first packed row of each image (multiple of IAMX_ROW_PAD)
 *   img_n    DEV [n_img] int32  valid rows of each image (>= 2 for a train image)
 *   pairs    DEV [n_pairs][2] int32  (query image, train image)
 *   wg_off   DEV [n_pairs+1] int32   exclusive scan of iamx_knn2_wg_per_pair(n_q)
 *   out_off  DEV [n_pairs] int64     first output row of each pair
 *   out_idx  DEV [sum n_q][2] int32  train row (0-based inside the train image)
 *   out_d2   DEV [sum n_q][2] int32  squared distances
 *   total_wg = wg_off[n_pairs] (HOST value)
 * ------------------------------------------------------------------------------------ */
int iamx_knn2_wg_per_pair(int n_query_rows);

int iamx_knn2_l2_pairs(const int8_t *desc, const int32_t *norm_q, const int32_t *norm_t,
                       const int32_t *img_off, const int32_t *img_n,
                       const int32_t *pairs, const int32_t *wg_off, const int64_t *out_off,
                       int n_pairs, int total_wg,
                       int32_t *out_idx, int32_t *out_d2, void *stream);

/* Single pair over two packed images (thin wrapper over the batched kernel).
 * q_*, t_*: DEV packed image (iamx_desc_pack_*); idx/d2: DEV [nq][2] int32. */
int iamx_knn2_l2_u8(const int8_t *q_desc, const int32_t *q_norm_q, int nq,
                    const int8_t *t_desc, const int32_t *t_norm_t, int nt,
                    int32_t *idx, int32_t *d2, void *stream);

/* K3: the exact 3-nearest-neighbour search of the 'smart' strategy -- replaces
 *   the_matcher.knnMatch(des1, des2, k=3)           scripts/lib/matcher.py:456-470
 * Every argument table is that of iamx_knn2_l2_pairs (wg_off from iamx_knn2_wg_per_pair too);
 *   out_idx / out_d2  DEV [sum n_q][3] int32, ascending by (squared distance, train row): equal
 *   distances go to the lower train row.  Columns 0-1 are what iamx_knn2_l2_pairs writes.
 * A train image of fewer than 3 rows leaves the missing neighbours as idx = -1, d2 = 0x7FFFFFFF
 * (cv2 returns a shorter list there: the reference's `for j in range(len(m))` then sees two). */
int iamx_knn3_l2_pairs(const int8_t *desc, const int32_t *norm_q, const int32_t *norm_t,
                       const int32_t *img_off, const int32_t *img_n,
                       const int32_t *pairs, const int32_t *wg_off, const int64_t *out_off,
                       int n_pairs, int total_wg,
                       int32_t *out_idx, int32_t *out_d2, void *stream);

/* ------------------------------------------------------------------------------------
 * Quality metric + threshold -- replaces the python loop scripts/lib/matcher.py:253-263:
 *     ratio = d0/d1 ; metric = d0*ratio ; keep metric < max_distance*match_ratio
 * with d0,d1 = float32 sqrt of the squared distances, the rest in float64 like python.
 *   idx,d2     DEV [n][2] int32  (output of iamx_knn2_*)
 *   seg_off    DEV [n_seg+1] int64  rows of each (ordered) pair inside idx/d2
 *   metric     DEV [n] float64     (all rows; NaN where d1 == 0 -> python raises there)
 *   keep       DEV [n] uint8
 *   seg_count  DEV [n_seg] int32   survivors per pair
 *   zero_div   DEV [1] int32       incremented for rows with d1 == 0 (matcher.py:255)
 * ------------------------------------------------------------------------------------ */
int iamx_match_metric(const int32_t *d2, const int64_t *seg_off, int n_seg, double thresh,
                      double *metric, uint8_t *keep, int32_t *seg_count, int32_t *zero_div,
                      void *stream);

/* Order-preserving compaction of the survivors of every pair.
 *   surv_off   DEV [n_seg+1] int64  exclusive scan of seg_count (caller computes it, or
 *                                   iamx_exclusive_scan_i32)
 *   surv_q/surv_t  DEV [sum seg_count] int32   query row / train row
 *   surv_metric    DEV [sum seg_count] float64 */
int iamx_match_compact(const int32_t *idx, int idx_stride, const double *metric,
                       const uint8_t *keep, const int64_t *seg_off, const int64_t *surv_off,
                       int n_seg, int32_t *surv_q, int32_t *surv_t, double *surv_metric,
                       void *stream);
/* (surv_t[k] = idx[idx_stride * row]: stride 2 reads the best index of iamx_knn2_l2_*, stride 1
 *  the tile ids of iamx_knn2v2_pairs, which iamx_knn2v2_resolve then turns into train rows) */

/* ------------------------------------------------------------------------------------
 * K2, fast form: top-2 DISTANCES without index tracking in the sweep; the train index is
 * recovered afterwards, only for the rows that survive the metric threshold.  Same survivor
 * lists as iamx_knn2_l2_pairs + iamx_match_metric + iamx_match_compact (tests pin that).
 *   exact_second = 1: out_d2 = exact (best, second) for every row (2 VALU ops / distance);
 *                     finish with iamx_match_metric/_compact + iamx_knn2v2_resolve.
 *   exact_second = 0: out_d2[.][1] is an UPPER BOUND of the second distance (smallest distance
 *                     outside the best's 16-row group; 0.75 VALU ops / distance).  Threshold
 *                     with it (iamx_match_metric/_compact keep a superset of the survivors),
 *                     then iamx_knn2v2_finish makes `second` exact for those rows (d2 updated
 *                     in place), re-applies the test, resolves the train rows and compacts
 *                     each pair's survivors in place: pair p owns
 *                     surv_*[surv_off[p] .. surv_off[p] + surv_cnt[p]).
 *
 * Train-side store ("desc2"): rows of an image stably partitioned by the parity of
 * NB = |a-128|^2 + 2*sum(a-128), each class zero-padded to 128 rows:
 *   rows_cap = iamx_desc2_rows_cap(n)   rows to reserve per image
 *   dst DEV [rows_cap][128] int8, norm2/cinit/perm DEV [rows_cap] int32 (perm = original row,
 *   -1 on padding), meta DEV [4] int32 = {n, even chunks, odd chunks, n_even}
 * Query side = the ordinary store of iamx_desc_pack_*.
 *   out_d2   DEV [sum n_q][2]  squared distances (best, second)
 *   out_tile DEV [sum n_q]     32-row tile of the packed train image holding the best row
 * iamx_knn2v2_resolve: surv_t holds tile ids on entry and train rows (original numbering,
 * lowest row among equal distances) on exit; n_unresolved counts internal inconsistencies (0).
 * ------------------------------------------------------------------------------------ */
int64_t iamx_desc2_rows_cap(int64_t n_rows);
/* scratch: DEV [3 * n_rows] int32 (3 * total_rows for the batch form).  Batch form: images
 * back to back in `src`, src_off DEV [n_img+1] int64 first source row, dst_off DEV [n_img]
 * int32 first packed row (multiples of 128, >= rows_cap apart), meta DEV [n_img][4]. */
int iamx_desc2_pack_u8(const uint8_t *src, int64_t n_rows, int8_t *dst, int32_t *norm2,
                       int32_t *cinit, int32_t *perm, int32_t *meta, int32_t *scratch,
                       void *stream);
int iamx_desc2_pack_f32(const float *src, int64_t n_rows, int8_t *dst, int32_t *norm2,
                        int32_t *cinit, int32_t *perm, int32_t *meta, int32_t *scratch,
                        void *stream);
int iamx_desc2_pack_batch_u8(const uint8_t *src, const int64_t *src_off, const int32_t *dst_off,
                             int n_img, int64_t total_rows, int max_rows_per_image, int8_t *dst,
                             int32_t *norm2, int32_t *cinit, int32_t *perm, int32_t *meta,
                             int32_t *scratch, void *stream);
int iamx_knn2v2_pairs(const int8_t *desc_q, const int32_t *norm_q, const int32_t *qimg_off,
                      const int32_t *qimg_n, const int8_t *desc_t, const int32_t *cinit,
                      const int32_t *timg_off, const int32_t *tmeta, const int32_t *pairs,
                      const int32_t *wg_off, const int64_t *out_off, int n_pairs, int total_wg,
                      int rows_per_wg /* 256, 512 or (exact_second = 0 only) 1024:
                                         wg_off = scan of ceil(n_q / rows_per_wg) */,
                      int exact_second, int32_t *out_d2, int32_t *out_tile, void *stream);
int iamx_knn2v2_resolve(const int8_t *desc_q, const int32_t *norm_q, const int32_t *qimg_off,
                        const int8_t *desc_t, const int32_t *norm2_t, const int32_t *perm,
                        const int32_t *timg_off, const int32_t *pairs, const int64_t *out_off,
                        const int32_t *d2, const int64_t *surv_off, const int32_t *surv_q,
                        int32_t *surv_t, int n_pairs, int32_t *n_unresolved, void *stream);
/* thresh: the same value as given to iamx_match_metric; zero_div is incremented for every row
 * whose exact second distance is 0 (scripts/lib/matcher.py:255 divides by it). */
int iamx_knn2v2_finish(const int8_t *desc_q, const int32_t *norm_q, const int32_t *qimg_off,
                       const int8_t *desc_t, const int32_t *norm2_t, const int32_t *perm,
                       const int32_t *timg_off, const int32_t *pairs, const int64_t *out_off,
                       int32_t *d2, double thresh, const int64_t *surv_off, int32_t *surv_q,
                       int32_t *surv_t, double *surv_metric, int32_t *surv_cnt, int n_pairs,
                       int32_t *zero_div, int32_t *n_unresolved, void *stream);

/* ------------------------------------------------------------------------------------
 * K2, symmetric form (shipped for batches that hold both directions of every image pair, which
 * is what bidirectional_pair_matches asks for, scripts/lib/matcher.py:304-347): ONE MFMA sweep
 * of the distance matrix of an unordered pair serves both directions.  The sweep only produces,
 * for every row of both images, a lower bound of the best and an upper bound of the second
 * squared distance; the reference's test d0*(d0/d1) < thresh (:253-263) is monotone in both,
 * so iamx_knn2sym_candidates keeps a superset of its survivors and iamx_knn2sym_exact
 * recomputes exactly those rows against the whole train image (lowest train row on ties, like
 * cv2.BFMatcher) and re-applies the test.  What leaves the path -- surv_q / surv_t /
 * surv_metric per ordered pair in ascending query order, d2 of the survivors, zero_div -- is
 * identical to iamx_knn2_l2_pairs + iamx_match_metric + iamx_match_compact.
 *
 * Store ("desc3"): the rows of an image sorted by sn2 = |a-128|^2 (stable), zero-padded to
 * rows_cap = iamx_desc3_rows_cap(n) (a multiple of 128) rows:
 *   dst DEV [rows_cap][128] int8; sn2 / sct / sperm / sinv DEV [rows_cap] int32 with
 *   sct = (sn2 + 2*sum(a-128)) >> 1 (2^30-ish on padding), sperm = original row of a sorted
 *   row (-1 on padding), sinv = sorted position of an original row.
 *   scratch DEV [3 * n_rows] int32 (3 * total_rows for the batch form, laid out like
 *   iamx_desc2_pack_batch_u8).
 * Sweep: upairs DEV [n_u][2] = (B image, A image): B rows stay in registers (1024 / 512 / 256
 * per workgroup for form 2 / 1 / 0 = iamx_knn2sym_rows_per_wg(form)), A rows stream through LDS.
 *   wg_off   DEV [n_u+1] int32  scan of ceil(n_B / rows_per_wg);  total_wg = wg_off[n_u]
 *   col_off  DEV [n_u] int64    first entry of pair u in col  (scan of rows_cap(B))
 *   rowp_off DEV [n_u] int64    first entry of pair u in rowp (scan of workgroups x rows_cap(A))
 *   col  DEV [..][2] int32, rowp DEV [..][2] int32 (8-byte aligned): the bounds, internal format
 * Candidates: pairs DEV [n_pairs][2] ordered (query image, train image); osrc DEV [n_pairs][2] =
 *   (index u of its unordered pair, role: 0 if the query image is B, 1 if it is A);
 *   out_off DEV [n_pairs+1] int64 rows of each ordered pair; keep DEV [max(rows, 8)] uint8 scratch
 *   (4-byte aligned; used as a bit map, one bit per query row of rows_total, cleared by the call);
 *   cand_cnt DEV [n_pairs] (written); cand_q DEV [rows]: the candidate query rows (original
 *   numbering, ascending) of pair p at out_off[p] .. + cand_cnt[p] -- a pair's list lives in
 *   its own slice of the row range, no scan over the pairs;
 *   d2 DEV [rows][2] int32 (the array iamx_knn2sym_exact fills): entry [r][1] of a candidate row
 *   receives an upper bound of its exact second squared distance, which the exact stage prunes its
 *   scan with before it replaces the pair of values.
 *   task_total DEV [2] (must be 0 on entry; iamx_knn2sym_exact leaves it 0), tasks DEV
 *   [2 n_pairs + rows/32 + 2][2]: the tasks (ordered pair, block) of the exact stage -- wave
 *   tasks (pairs with <= 64 candidates) from entry 0, workgroup tasks (256 candidates) from
 *   entry n_pairs.
 * Exact: desc / norm_q / norm_t / img_off = the ORIGINAL-order store of iamx_desc_pack_*.  A
 *   wave task: <= 64 candidates x the whole train image on the MFMA, train tiles straight from
 *   L2; a workgroup task: 4 x 64 candidates, every train tile staged once in LDS for the four
 *   waves (the form real frames need: a third to two thirds of a pair's rows are candidates
 *   there, against 0.1 % on uncorrelated synthetic descriptors).  Writes d2 DEV [rows][2]
 *   for the candidate rows, then compacts every pair's list in place to its survivors: pair p
 *   owns cand_q / cand_t / cand_metric [out_off[p] .. + surv_cnt[p]); zero_div is incremented
 *   for every row whose exact second distance is 0 (matcher.py:255 divides by it).
 * ------------------------------------------------------------------------------------ */
int64_t iamx_desc3_rows_cap(int64_t n_rows);
int iamx_knn2sym_rows_per_wg(int form);
/* the sweep kernel a form launches, spelled the way rocprofv3 prints it ("knn2sym_kernel<4, 8, ...>"):
 * profile summaries are matched against the binary that is loaded (bench.py refuses stale ones) */
const char *iamx_knn2sym_kernel_id(int form);
int iamx_desc3_pack_u8(const uint8_t *src, int64_t n_rows, int8_t *dst, int32_t *sn2,
                       int32_t *sct, int32_t *sperm, int32_t *sinv, int32_t *scratch,
                       void *stream);
int iamx_desc3_pack_f32(const float *src, int64_t n_rows, int8_t *dst, int32_t *sn2,
                        int32_t *sct, int32_t *sperm, int32_t *sinv, int32_t *scratch,
                        void *stream);
int iamx_desc3_pack_batch_u8(const uint8_t *src, const int64_t *src_off, const int32_t *dst_off,
                             int n_img, int64_t total_rows, int max_rows_per_image, int8_t *dst,
                             int32_t *sn2, int32_t *sct, int32_t *sperm, int32_t *sinv,
                             int32_t *scratch, void *stream);
/* Narrow exact stage (round 6).  The sweep knows WHERE a candidate's two smallest distances can
 * be: a query that was a B row has eight group minima over the streamed image (group = (32-row
 * tile & 3, lane half): colmask DEV [col rows] uint8 receives the groups whose minimum is <= v2),
 * a query that was an A row one (L, U1, U2) per row block of the register-resident image (block w
 * can hold a row at or below the upper bound of the second distance only if L_w <= U2).  With
 * nar != NULL (DEV, iamx_knn2sym_narrow_bytes(rows_total, n_pairs) bytes, rows_total = rows of
 * all ordered pairs = out_off[n_pairs]; its first 256 bytes must be 0 on the first call, the exact
 * stage leaves them 0) iamx_knn2sym_candidates turns the candidates of every ordered pair with more
 * than 64 of them (train image >= 1024 rows, <= 64 row blocks) into items (candidate, class) bucketed
 * by class, and iamx_knn2sym_exact scans ONE class per task -- 1/8 of the train image (column
 * direction) or one row block (row direction) instead of all of it -- and merges a candidate's
 * items.  Results are those of the full scan: every row that can be the best, the second or tied
 * with either lies in a class of the candidate's mask.  Pairs whose items do not fit the buffer take
 * the full scan.  The same nar / colmask / form must be given to both calls; nar == NULL (or the
 * environment switch IAMX_EXACT_NARROW=0, read by both) = full scan for every pair. */
int64_t iamx_knn2sym_narrow_bytes(int64_t rows_total, int n_pairs);
int iamx_knn2sym_sweep(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                       const int32_t *img_off, const int32_t *img_n, const int32_t *upairs,
                       const int32_t *wg_off, const int64_t *col_off, const int64_t *rowp_off,
                       int n_u, int total_wg, int form, int32_t *col, int32_t *rowp,
                       uint8_t *colmask /* may be NULL */, void *stream);
/* iamx_knn2sym_sweep for form 2 with the pairs dealt as ITEMS: items DEV [n_items][3] int32 =
 * (first unordered pair, pair count, B slice = workgroup index within the pair), one workgroup per
 * item; every pair of an item has the same number of 1024-row B slices, and the pairs should be
 * sorted by B image (the B slice is loaded again only where the image changes).  col, rowp and
 * colmask are those of iamx_knn2sym_sweep with form 2 for the same upairs / col_off / rowp_off,
 * bit for bit (kernels.sym_items builds the table). */
int iamx_knn2sym_sweep_items(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                             const int32_t *img_off, const int32_t *img_n, const int32_t *upairs,
                             const int32_t *items, const int64_t *col_off, const int64_t *rowp_off,
                             int n_u, int n_items, int32_t *col, int32_t *rowp,
                             uint8_t *colmask /* may be NULL */, void *stream);
/* iamx_knn2sym_sweep_items on v_mfma_i32_16x16x64_i8 (the shape the chip clocks higher): the same
 * arguments, the same col, rowp and colmask bit for bit; iamx_knn2sym_items16_kernel_id() is its
 * kernel's name the way rocprofv3 prints it. */
int iamx_knn2sym_sweep_items16(const int8_t *sdesc, const int32_t *sn2, const int32_t *sct,
                               const int32_t *img_off, const int32_t *img_n, const int32_t *upairs,
                               const int32_t *items, const int64_t *col_off, const int64_t *rowp_off,
                               int n_u, int n_items, int32_t *col, int32_t *rowp,
                               uint8_t *colmask /* may be NULL */, void *stream);
const char *iamx_knn2sym_items16_kernel_id(void);
/* iamx_knn2sym_candidates reads sn2, col and rowp 16 bytes (four sorted rows) at a time: img_off
 * (= img_off3 of the sorted store), col_off and rowp_off must be multiples of 4 rows, every image's
 * slice of sn2 / col and every workgroup's slice of rowp padded to iamx_desc3_rows_cap(n) rows, and the
 * three arrays 16-byte aligned -- what the sweep's own layout (caps of 128 rows) gives.  cand_cnt
 * DEV [n_pairs] is cleared by the call and ends holding every pair's candidate count. */
int iamx_knn2sym_candidates(const int32_t *sn2, const int32_t *sperm, const int32_t *img_off,
                            const int32_t *img_n, const int32_t *pairs, const int32_t *osrc,
                            const int32_t *wg_off, const int64_t *col_off, const int64_t *rowp_off,
                            const int64_t *out_off, const int32_t *col, const int32_t *rowp,
                            int n_pairs, double thresh, uint8_t *keep, int32_t *cand_cnt,
                            int32_t *cand_q, int32_t *task_total, int32_t *tasks, int32_t *d2,
                            const uint8_t *colmask, void *nar /* may be NULL */, int64_t rows_total,
                            int max_query_rows /* rows of the largest query image */, int form,
                            void *stream);
/* key_t DEV [total_rows] int32 scratch beside norm_t (total_rows = rows of the whole original-
 * order store): rewritten by every call with the per-row constant of the packed (distance, row)
 * key.  task_total DEV [2], tasks DEV [2 n_pairs + rows / 32 + 2][2] (iamx_knn2sym_candidates
 * fills them: a pair with <= 64 candidates is one WAVE task, entries from 0; a pair with more
 * gets WORKGROUP tasks of 256 candidates, entries from n_pairs -- four waves share every train
 * tile through LDS; both counters are reset by this call).  sdesc / sn2 / sct / sperm / img_off3 =
 * the SORTED store of the sweep, osrc as for iamx_knn2sym_candidates: read by the narrow stage only
 * (may be NULL with nar == NULL). */
int iamx_knn2sym_exact(const int8_t *desc, const int32_t *norm_q, const int32_t *norm_t,
                       int32_t *key_t, int64_t total_rows,
                       const int32_t *img_off, const int32_t *img_n, const int32_t *pairs,
                       const int64_t *out_off, const int32_t *cand_cnt, int32_t *task_total,
                       const int32_t *tasks, int32_t *cand_q, int n_pairs, double thresh,
                       int32_t *d2, int32_t *cand_t, double *cand_metric, uint8_t *cand_keep,
                       int32_t *surv_cnt, int32_t *zero_div, const int8_t *sdesc,
                       const int32_t *sn2, const int32_t *sct, const int32_t *sperm,
                       const int32_t *img_off3, const int32_t *osrc, void *nar /* may be NULL */,
                       int64_t rows_total, int form, void *stream);

/* ------------------------------------------------------------------------------------
 * Per-pair match filters on the device, both directions of n_pairs image pairs, one workgroup
 * per pair -- replaces the python between the metric threshold and find_matches' bookkeeping:
 *   scripts/lib/matcher.py:258-269 (stable sort by metric, clip 2000), :271-283 (< min_pairs),
 *   :285 cv2.xfeatures2d.matchGMS(withRotation=True, withScale=False, thresholdFactor),
 *   :157-182 filter_duplicates, :296-299, :304-318 (reverse only if forward kept >= min_pairs),
 *   :187-200 filter_cross_check.
 * Ordered pair k (k < n_pairs) is the forward direction of pair k, ordered pair n_pairs + k its
 * reverse: surv_off DEV [2 n_pairs + 1], surv_cnt DEV [2 n_pairs], pairs DEV [2 n_pairs][2]
 * (image slots) and surv_q/_t/_metric are the outputs of the matching stage.
 *   kp_off DEV [n_images] int64   first keypoint of an image slot in xy / key2
 *   xy     DEV [total kp][2] f32  kp.pt (full-res pixels, inside [0,width) x [0,height))
 *   key2   DEV [total kp][2] i32  round-half-even(100 * kp.pt): the "%.2f" keys of :166-167
 *   out_cnt DEV [n_pairs], out_pairs DEV [n_pairs][clip][2]: the cross-checked forward list
 *   [query row, train row] (the reverse list is its mirror); scratch DEV [n_pairs][2][clip][2];
 *   out_stat DEV [n_pairs][4]: forward after GMS / after de-dup, reverse after GMS / after
 *   de-dup (-1 = stage not reached); status DEV [n_pairs]: 1 = a direction has more than 2^24
 *   survivors (out_cnt 0): the caller refuses the batch -- an image of at most 2^24 rows
 *   cannot cause it.  clip = iamx_match_postfilter_clip() = 2000.
 * ------------------------------------------------------------------------------------ */
int iamx_match_postfilter_clip(void);
/* The per-pair results of a batch packed back to back (what find_matches downloads: on an
 * all-pairs schedule almost every pair ends with nothing and the [n_pairs][clip] slots are 130 MB
 * per 4096 pairs).  cnt / status / pairs as written by iamx_match_postfilter, z DEV
 * [n_pairs][clip] of iamx_triangulate_pairs or NULL.  off [n_pairs + 1] int64: exclusive scan of
 * the counts of the pairs with status 0 (off[n_pairs] = total); out_pairs [cap][2], out_z [cap]
 * (NULL without z): pair k's rows at [off[k], off[k] + cnt[k]) when off[k] + cnt[k] <= cap.
 * off / out_pairs / out_z may be page-locked HOST memory (written by the device directly). */
int iamx_match_pack_results(const int32_t *cnt, const int32_t *status, const int32_t *pairs,
                            const double *z, int n_pairs, int clip, int64_t cap, int64_t *off,
                            int32_t *out_pairs, double *out_z, void *stream);
int iamx_match_postfilter(const int64_t *surv_off, const int32_t *surv_cnt, const int32_t *surv_q,
                          const int32_t *surv_t, const double *surv_metric, const int32_t *pairs,
                          const int64_t *kp_off, const float *xy, const int32_t *key2, int n_pairs,
                          double width, double height, double min_pairs, double threshold_factor,
                          int32_t *out_cnt, int32_t *out_pairs, int32_t *scratch,
                          int32_t *out_stat, int32_t *status, void *stream);

/* iamx_thp_pays -- HOST.  1 when MADV_HUGEPAGE speeds up the first touch of fresh anonymous memory
 * on this host right now, 0 when it slows it down (a fragmented host makes every such fault wait
 * for the kernel's compaction); probed once per process with 2 x 32 MiB, IAMX_THP=0 / 1 overrides.
 * The work arrays of iamx_link_matches and the package's result arrays (matchpairs.empty_huge,
 * what find_matches' rounds land in: scripts/lib/matcher.py:918-1031) go by it. */
int iamx_thp_pays(void);

/* ------------------------------------------------------------------------------------
 * match consolidation (host) and initial triangulation (device).
 *
 * iamx_link_matches -- scripts/lib/match_cleanup.py:246-301 link_matches(): HOST arrays in and
 *   out (no device involved).  Chain i of the input = points [ptr[i], ptr[i+1]) of (img[],
 *   kp[]); the linked chains come back in the reference's order (the caller sorts by length),
 *   out arrays sized like the input.  Returns the number of chains or a negative error code.
 * iamx_triangulate_ground -- match_cleanup.py:320-347 triangulate_smart(): per feature the mean
 *   of the ground-plane intersections of its observation rays.
 *   M DEV [n_images][9] = (body2ned . cam2body) . inv(K) row major, ned DEV [n_images][3],
 *   base_elev DEV [n_images], obs_img DEV [n_obs] int32, obs_uv DEV [n_obs][2] f64,
 *   feat_ptr DEV [n_feat+1] int64, out_ned DEV [n_feat][3], n_sky DEV [1] (+= rays that point
 *   above the horizon; they add nothing to the sum but count in the divisor, like the reference)
 * ------------------------------------------------------------------------------------ */
int64_t iamx_link_matches(const int32_t *img, const int32_t *kp, const int64_t *ptr,
                          int64_t n_matches, int32_t *out_img, int32_t *out_kp, int64_t *out_ptr,
                          int32_t *n_passes);
/* iamx_link_pair_blocks -- the same for the pair matches of make_match_structure()
 * (match_cleanup.py:190-215) handed over as they lie in the images' match lists: blocks[b] = HOST
 * int32 [counts[b]][2] (keypoint of image ij[2b], keypoint of image ij[2b+1]), pairs in the
 * reference's order; out arrays hold 2 * sum(counts) points / sum(counts) + 1 offsets. */
int64_t iamx_link_pair_blocks(const int32_t *const *blocks, const int64_t *counts, const int32_t *ij,
                              int64_t n_blocks, int32_t *out_img, int32_t *out_kp, int64_t *out_ptr,
                              int32_t *n_passes);
/* iamx_chain_members_uv -- HOST.  The "replace keypoint indices with uv coordinates" step of
 * link_matches (scripts/lib/match_cleanup.py:277-287) for all chain members at once: uv[k] =
 * (double) kp.pt of keypoint f_kp[k] of image f_img[k], from the images' own position arrays
 * (xy[i] float32 [n_kp[i]][2]).  Negative indices count from the end like a python list's; an index
 * outside the image's list -> IAMX_EINVAL, *bad_member = the first such member. */
int iamx_chain_members_uv(const int32_t *f_img, const int32_t *f_kp, int64_t n_members,
                          const float *const *xy, const int64_t *n_kp, int32_t n_images, double *uv,
                          int64_t *bad_member, int threads);
/* iamx_kp_key2 -- HOST.  key2[k] = round-half-even(100 * xy[k]) in exact integer arithmetic: the
 * "%.2f-%.2f" % kp.pt keys of scripts/lib/matcher.py:166-167 and match_cleanup.py:36-38 as integer
 * pairs (xy float32 [n][2] in [0, 16384), key2 int32 [n][2]).
 * iamx_kp_dup_remap -- HOST.  merge_duplicates' per-image table (match_cleanup.py:19-60) for
 * n_images images at once: remap[k] (index inside the image) = the first USED keypoint of the
 * image with keypoint k's key, k itself when k is unused; identity[i] = 1 when image i has no two
 * used keypoints on one pixel.  Flat arrays, image i at [kp_base[i], kp_base[i+1]). */
int iamx_kp_key2(const float *xy, int64_t n, int32_t *key2);
int iamx_kp_dup_remap(const float *xy, const uint8_t *used, const int64_t *kp_base, int32_t n_images,
                      int32_t *remap, uint8_t *identity, int threads);
/* iamx_match_lists_scan -- HOST.  One pass over the images' match lists for the per-list loops in
 * front of link_matches (scripts/lib/match_cleanup.py:19-188, lib/project.py:331-350
 * compute_kp_usage): list b = int32 [cnt[b]][2] (keypoint of image ia[b], keypoint of image ib[b]),
 * keypoints of image i at [kp_base[i], kp_base[i+1]) of the flat arrays `used` (uint8) / `remap`.
 * mode & 1: mark both keypoints used; & 2: replace both by remap[...] in place (merge_duplicates);
 * & 4: dup_pairs[b] = rows equal to an earlier row, dup_first[b] = rows whose first keypoint
 * occurred before (check_for_pair_dups / check_for_1vn_dups).  A keypoint index outside its image
 * is IAMX_EINVAL (the reference raises IndexError there). */
int iamx_match_lists_scan(int32_t *const *lists, const int64_t *cnt, const int32_t *ia,
                          const int32_t *ib, int64_t n_lists, const int64_t *kp_base, int32_t n_images,
                          uint8_t *used, const int32_t *remap, int mode, int32_t *dup_pairs,
                          int32_t *dup_first, int threads);
/* HOST helpers of the same stage.  iamx_chains_longest_first: the chains of iamx_link_matches in
 * the order match_cleanup.py:291-292 leaves them (stable sort by length, longest first), members
 * copied on `threads` threads; out arrays sized like the input, out_ptr [n_chains + 1].
 * iamx_first_occurrence: first[k] = smallest j with key[j] == key[k] (merge_duplicates,
 * match_cleanup.py:19-104: keypoints of an image on the same pixel collapse onto the first). */
int iamx_chains_longest_first(const int32_t *img, const int32_t *kp, const int64_t *ptr,
                              int64_t n_chains, int32_t *out_img, int32_t *out_kp, int64_t *out_ptr,
                              int threads);
int iamx_first_occurrence(const int64_t *key, int64_t n, int64_t *first);
/* iamx_ledger_index -- HOST arrays.  matcher.find_matches (scripts/lib/matcher.py:978-979) gives
 * BOTH images of every processed pair a match_list entry, in processing order; for the pairs
 * without matches -- 95-99 % of an all-pairs schedule -- this package keeps index arrays (qi, qj,
 * seq ascending) and this routine turns them into the per-image lists the .match writer walks:
 * image k's partners and their seq at [bounds[k], bounds[k+1]) of other / seq_out (2 m entries),
 * bounds [n_images + 1].  One counting sort. */
int iamx_ledger_index(const int64_t *qi, const int64_t *qj, const int64_t *seq, int64_t m,
                      int64_t n_images, int64_t *other, int64_t *seq_out, int64_t *bounds);
/* iamx_pairs_fwd_rev, iamx_segment_mean_std -- HOST arrays, `threads` host threads.  The bulk
 * work of one round of find_matches between the device's packed result buffer and the match
 * lists of scripts/lib/matcher.py:978-979: fwd = the n (query, train) int32 rows copied out of the
 * page-locked buffer, rev = the same rows with the columns swapped (the list of the reversed
 * direction); and, per pair, the mean and standard deviation of its triangulated heights
 * (lib/smart.py:117-130 estimate_surface_elevation: np.mean / np.std of the pair's values) over
 * the segments z[starts[s] .. + counts[s]) of the round's packed heights, summed in numpy's
 * order. */
int iamx_pairs_fwd_rev(const int32_t *src, int64_t n, int32_t *fwd, int32_t *rev, int threads);
/* reads one byte of every 4 KiB page of a HOST buffer on `threads` threads (first touch of the
 * page-locked landing buffers of find_matches' rounds, off the critical path) */
int iamx_touch_pages(const void *p, int64_t bytes, int threads);
int iamx_segment_mean_std(const double *z, const int64_t *starts, const int64_t *counts,
                          int64_t n_seg, int64_t n_z, double *mean, double *std, int threads);

/* iamx_hbm_copy16 -- measurement yardstick of the HBM-bound kernels (bench.py, tools/): a plain
 * grid-stride device kernel that writes n16 16-byte words, each the sum of reads_per_write (1..4)
 * source words (src holds reads_per_write x n16 words: 1 = a copy, 3 = the read : write mix of the
 * BA residual kernel), 16 bytes per lane and step, `workgroups` x 256 threads.  No counterpart in
 * the reference. */
int iamx_hbm_copy16(const void *src, void *dst, int64_t n16, int reads_per_write, int workgroups,
                    void *stream);

/* iamx_yaw_feedback_* -- the yaw-error FEEDBACK of the reference's pair loop as a prefix
 * computation over the schedule (HOST code).  scripts/lib/matcher.py:987-993 sets both images'
 * aircraft yaw-error estimate after every pair (lib/smart.py:251-283 update_yaw_error_estimate:
 * 0 without matches / without a similarity fit, else the weighted average over the image's
 * yaw_pairs entries -- values rounded through "%.1f", weights truncated like getInt, children in
 * sorted-name order, entries closer than 0.5 m or more than 30 degrees off skipped), and
 * lib/image.py:434-457 turns it into the camera pose the image's NEXT pair triangulates with.
 * _new: name_rank [n_images] rank of every image's name in sorted order; _seed: entries an image's
 * yaw_pairs node holds before the call; _feed: one round in schedule order (see the definition);
 * _state: every image's current estimate and whether a pair of the call has touched it. */
void *iamx_yaw_feedback_new(int n_images, const int32_t *name_rank);
void iamx_yaw_feedback_free(void *h);
int iamx_yaw_feedback_seed(void *h, int image, int n, const int32_t *partner_image, const double *err,
                           const double *weight, const double *dist);
int iamx_yaw_feedback_feed(void *h, int64_t n, const int32_t *pi, const int32_t *pj,
                           const uint8_t *quiet, int64_t n_hits, const int64_t *hit_rows,
                           const double *yv_f, const double *yv_r, const uint8_t *ok, double *e1,
                           double *e2, uint8_t *fresh1, uint8_t *fresh2);
int iamx_yaw_feedback_state(void *h, double *value, uint8_t *touched);

/* iamx_group_level -- one group level of scripts/lib/groups.py:59-118 compute() (HOST arrays):
 * seed chain + sweeps until nothing can be added.  level [n_matches] in/out (-1 = unused),
 * placed_images [n_images] 0/1 from earlier levels, placed_matches [n_images] out.  Returns the
 * seed chain index, -1 if there is none, or a negative error code < -1. */
int64_t iamx_group_level(const int32_t *img, const int64_t *ptr, int64_t n_matches, int n_images,
                         int32_t *level, const uint8_t *placed_images, int group_level,
                         int use_single_pairs, int max_wanted, int min_connections,
                         int32_t *placed_matches);
int iamx_triangulate_ground(const double *M, const double *ned, const double *base_elev,
                            int n_images, const int32_t *obs_img, const double *obs_uv,
                            const int64_t *feat_ptr, int64_t n_feat, double *out_ned,
                            int32_t *n_sky, void *stream);

/* iamx_triangulate_pairs -- scripts/lib/smart.py:26-63 triangulate_features(): two-view linear
 * (DLT) triangulation of the matches of every pair of a batch, what cv2.triangulatePoints
 * computes (null direction of the 4x4 system, f64), w-normalised; only the NED "down" component
 * is returned because estimate_surface_elevation() (:117-130) needs nothing else.
 *   pair_img DEV [n_pairs][2] image slots, PROJ DEV [n_images][12] = [R | t] row major,
 *   IK DEV [9] inverse camera matrix, kp_off / xy as for iamx_match_postfilter,
 *   m_cnt DEV [n_pairs], m_pairs DEV [n_pairs][clip][2] (query row, train row),
 *   out_z DEV [n_pairs][clip] */
int iamx_triangulate_pairs(const int32_t *pair_img, const double *PROJ, const double *IK,
                           const int64_t *kp_off, const float *xy, const int32_t *m_cnt,
                           const int32_t *m_pairs, int n_pairs, int clip, double *out_z,
                           void *stream);

/* iamx_triangulate_pairs_xyz -- the same triangulation with all three w-normalised NED components,
 * what `points /= points[3]` leaves in rows 0..2 of triangulate_features()'s 4xN return value
 * (scripts/lib/smart.py:61-63); out_xyz DEV [n_pairs][clip][3] */
int iamx_triangulate_pairs_xyz(const int32_t *pair_img, const double *PROJ, const double *IK,
                               const int64_t *kp_off, const float *xy, const int32_t *m_cnt,
                               const int32_t *m_pairs, int n_pairs, int clip, double *out_xyz,
                               void *stream);

/* iamx_triangulate_packed -- the triangulation of iamx_triangulate_pairs over PACKED match lists
 * with one pair of projection matrices PER PAIR: the surface stage of find_matches.  The reference
 * rewrites both images' camera poses after every pair (scripts/lib/matcher.py:990-993 ->
 * lib/image.py:434-457 set_aircraft_yaw_error_estimate) and the next pair triangulates with them
 * (lib/smart.py:26-63 via lib/image.py:542-553 get_proj); the host replays that chain in schedule
 * order and passes every pair the two matrices the reference would have used.
 *   pair_img  DEV [n_pairs][2] image slots (kp_off / xy as above)
 *   pair_proj DEV [n_pairs][2][12] float64 row-major [R | t] of image 1 / image 2 of the pair
 *   m_off     DEV [n_pairs + 1] int64 first match of every pair; m_pairs DEV [total][2]
 *   out_z     DEV [total] NED "down" of every match (w-normalised) */
int iamx_triangulate_packed(const int32_t *pair_img, const double *pair_proj, const double *IK,
                            const int64_t *kp_off, const float *xy, const int64_t *m_off,
                            const int32_t *m_pairs, int n_pairs, int64_t total, double *out_z,
                            void *stream);

/* iamx_similarity_pairs -- scripts/lib/smart.py:66-89 find_affine(): the 2x3 similarity
 * (rotation, uniform scale, translation) between the matched keypoints of every pair of a batch,
 * for estimate_yaw_error() (:138-192).  The reference asks cv2.estimateAffinePartial2D (RANSAC);
 * this is a deterministic robust fit instead: least squares on all matches, then nine re-fits on
 * the matches within 200, 50, 10, 3, 3, ... px of the current model.
 *   pair_img / kp_off / xy / m_cnt / m_pairs / clip as for iamx_triangulate_pairs
 *   out_aff DEV [n_pairs][2][6] float64 row major: [p][0] maps image b's pixels onto image a's
 *   (find_affine(a, b)), [p][1] the other way; out_ok DEV [n_pairs][2]: 1 = a fit exists
 *   (>= 2 matches that do not coincide) */
int iamx_similarity_pairs(const int32_t *pair_img, const int64_t *kp_off, const float *xy,
                          const int32_t *m_cnt, const int32_t *m_pairs, int n_pairs, int clip,
                          double *out_aff, int32_t *out_ok, void *stream);

/* out[i] = sum_{j<i} in[j], out[n] = total; in DEV [n] int32, out DEV [n+1] int64 */
int iamx_exclusive_scan_i32(const int32_t *in, int64_t n, int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------
 * K3: bundle-adjustment reprojection residual -- replaces Optimizer.fun
 *   scripts/lib/optimizer.py:174-229 (per-camera cv2.projectPoints + concatenate).
 *   cams    DEV [n_cams][7] float64  ned(3), quat w,x,y,z (unnormalised; :326-328)
 *   pts     DEV [n_pts][3]  float64
 *   cam_idx / pt_idx  DEV [n_obs] int32   camera-major observation list (:397-404)
 *   uv      DEV [n_obs][2] float64   observed (distorted, full-res px; :383)
 *   calib   DEV [9] float64  fx, fy, cu, cv, k1, k2, p1, p2, k3   (lib/camera.py:94)
 *   r       DEV [2*n_obs] float64   (du0, dv0, du1, dv1, ...) = observed - projected
 * ------------------------------------------------------------------------------------ */
int iamx_ba_residual(const double *cams, int n_cams, const double *pts, int n_pts,
                     const int32_t *cam_idx, const int32_t *pt_idx, const double *uv,
                     int64_t n_obs, const double *calib, double *r, void *stream);

/* Same residual, faster form: each workgroup (512 observations, two per thread) builds the
 * rotation/position blocks of the cameras it touches in LDS first, then does 9 FMAs, one
 * reciprocal and the distortion polynomial per observation.  Fastest with camera-major
 * cam_idx (any order is legal).  uv and r must be 32-byte aligned, cam_idx and pt_idx 8-byte
 * aligned; cam_scratch is unused (may be NULL).  Results agree with iamx_ba_residual to
 * rounding. */
int iamx_ba_residual_prepared(const double *cams, int n_cams, const double *pts, int n_pts,
                              const int32_t *cam_idx, const int32_t *pt_idx, const double *uv,
                              int64_t n_obs, const double *calib, double *cam_scratch, double *r,
                              void *stream);

/* Residual + analytic Jacobian blocks (the reference has only finite differences:
 * scripts/lib/optimizer.py:142-169,491-501).  d r / d params, row-major per observation:
 *   Jc  DEV [n_obs][2][7]   wrt that observation's camera (ned, quat)
 *   Jp  DEV [n_obs][2][3]   wrt its 3-D point
 *   Jk  DEV [n_obs][2][8] or NULL   wrt (f, cu, cv, k1, k2, p1, p2, k3) with fx=fy=f
 *                                   ('global' calibration, optimizer.py:181-189)
 *   r may be NULL. */
int iamx_ba_residual_jac(const double *cams, int n_cams, const double *pts, int n_pts,
                         const int32_t *cam_idx, const int32_t *pt_idx, const double *uv,
                         int64_t n_obs, const double *calib, double *r,
                         double *Jc, double *Jp, double *Jk, void *stream);

/* Reprojection-error report (scripts/4b-mre-by-image.py:60-110), pass 1 of 2.  Inputs as for
 * iamx_ba_residual (camera-major observations), plus
 *   cam_ptr   DEV [n_cams+1] int64   camera c owns observations [cam_ptr[c], cam_ptr[c+1])
 *             (non-decreasing, cam_ptr[n_cams] = n_obs; values are clamped to [0, n_obs])
 * Per observation (du, dv) is formed with the arithmetic of iamx_ba_residual and
 * e = sqrt(du*du + dv*dv) with a separately rounded multiply and add (np.linalg.norm).
 * The residual vector itself is not written.  Outputs:
 *   cam_stats DEV [n_cams][3] float64  (mean e, max e, count); a camera without observations
 *             has count 0 and mean = max = 0 (the reference reports it as 9999.0)
 *   part      DEV [n_cams][8] float64  workspace (per-camera partials)
 *   summary   DEV [16] float64: [0] n_obs  [1] sum e  [2] sum e / n_obs  [3] mean |r|
 *             [4] std r (population)  [5] max |r|  [6] mean r  [7] cameras without observations
 *             (r = the 2*n_obs signed residuals; [8..10] belong to iamx_ba_mark_outliers)
 *   e         DEV [n_obs] float64 or NULL
 * Sums are reduced in a fixed order (no floating-point atomics): results are identical run to
 * run.  n_obs = 0 is legal (summary [2..6] NaN or 0/0).  uv 16-byte aligned, the other arrays
 * 8-byte aligned.  Two launches, no host synchronisation. */
int iamx_ba_reproj_stats(const double *cams, int n_cams, const double *pts, int n_pts,
                         const int32_t *cam_idx, const int32_t *pt_idx, const double *uv,
                         int64_t n_obs, const double *calib, const int64_t *cam_ptr,
                         double *cam_stats, double *part, double *summary, double *e,
                         void *stream);

/* Pass 2 (mark_outliers, 4b-mre-by-image.py:112-150): from e DEV [n_obs] and summary[2] (the
 * device-side mre) of pass 1,
 *   stddev = sqrt(sum (mre - e)^2 / n_obs)            -> summary[8]
 *   thr    = mre + stddev * trim_stddev               -> summary[9]
 * an observation is flagged when e > thr, or has_max != 0 and e > max_error.  The flagged
 * observation indices are written in ascending order to idx_out DEV [cap] int64, their e to
 * e_sel DEV [cap] float64 (the first min(count, cap) of them); count -> summary[10] (a float64,
 * exact).  work DEV [max(1, 3 * ceil(n_obs / 2048))] float64.  Every odd, small or empty n_obs
 * is legal (n_obs = 0: count 0, stddev NaN).  All pointers 8-byte aligned; idx_out / e_sel may
 * be NULL when cap = 0.  Five launches, no host synchronisation, fixed-order reductions. */
int iamx_ba_mark_outliers(const double *e, int64_t n_obs, double trim_stddev, int has_max,
                          double max_error, double *summary, double *work, int64_t *idx_out,
                          double *e_sel, int64_t cap, void *stream);

/* ------------------------------------------------------------------------------------
 * Image preparation -- replaces the cv2 calls of Image.load_rgb(equalize=True) and the resize
 * in detect_features (scripts/lib/image.py:105-112,313): BGR->HSV, CLAHE(clip_limit, 8x8) on
 * V, HSV->BGR, cv2.resize(fx=fy=scale, INTER_LINEAR).
 *   bgr  DEV [height][width][3] uint8;  out  DEV [out_h][out_w][3] uint8 with
 *   (out_h, out_w) = iamx_image_resized_dims = round(size*scale);  equalize = 0 skips CLAHE.
 * ------------------------------------------------------------------------------------ */
int64_t iamx_image_prep_workspace_bytes(int height, int width);
int iamx_image_resized_dims(int height, int width, double scale, int *out_h, int *out_w);
int iamx_image_equalize_resize(const uint8_t *bgr, int height, int width, int equalize,
                               float clip_limit, double scale, void *workspace,
                               int64_t workspace_bytes, uint8_t *out, void *stream);

/* Where a stage's result lives inside the workspace after iamx_image_equalize_resize with
 * equalize != 0 (tests / diagnosis; host only): stage 0 = hsv uint8 [height][width][3],
 * 1 = equalised BGR uint8 [height][width][3], 2 = tile histograms int32 [64][256] (row = tile
 * ty * 8 + tx, over the reflect-101 padded tile), 3 = tile look-up tables uint8 [64][256]; at
 * workspace + *offset, *bytes long.  Any other stage, or a null pointer, fails with -1. */
int iamx_image_prep_stage(int height, int width, int stage, int64_t *offset, int64_t *bytes);

/* ------------------------------------------------------------------------------------
 * Area downscale -- replaces cv2.resize(src, (0,0), fx, fy, interpolation=cv2.INTER_AREA) of the
 * texture step (scripts/lib/panda3d.py:38-41,69-72) for interleaved uint8 images.
 *   src  DEV [height][width][channels] uint8, channels 1 or 3;
 *   out  DEV [out_h][out_w][channels] uint8 with (out_h, out_w) = iamx_image_area_dims =
 *        round-half-even(height*fy), round-half-even(width*fx).
 * Per axis scale = 1.0/f (double).  OpenCV's published area algorithm for uint8 with a float work
 * type: float32 tap weights, x taps summed in order from 0 into a row buffer, rows combined in
 * order, multiply and add rounded separately, result rounded half to even; the integer branch
 * (block sum * float32(1/area), (sum + 2) >> 2 for 2x2, (float)sum / count over an edge) when
 * both scales are integers within DBL_EPSILON.  tests/area_restatement.py states it in numpy.
 * Downscale only: 1/fx < 1 or 1/fy < 1 is IAMX_EINVAL, and so is a scale above 4096.  One launch
 * on `stream`, no workspace, no host synchronisation.
 * ------------------------------------------------------------------------------------ */
int iamx_image_area_dims(int height, int width, double fx, double fy, int *out_h, int *out_w);
int iamx_image_resize_area(const uint8_t *src, int height, int width, int channels, double fx,
                           double fy, uint8_t *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Colour tables of the explorer -- replace the host loops of scripts/lib/histogram.py
 * (get_histogram_rgb, match_neighbors) and scripts/99-vignette.py (the survey's mean frame, the
 * radial fit's sums, the fitted mask, the mask's finish).  Frames are DEV [h][w][3] uint8,
 * interleaved, in the decoder's channel order; n_pixels = h*w, n_values = 3*h*w.  Every call
 * enqueues on `stream` and does not synchronise the host.  16-byte aligned images are read 48 bytes
 * (16 pixels) per lane and step; unaligned ones byte by byte, with the same results.
 *
 * iamx_colour_histogram: hist DEV uint32 [3][256] += the counts of img's three channels (the
 *   caller zeroes it once).  Integer counters throughout: LDS copies per workgroup, one integer
 *   global atomic per non-empty bin and workgroup.  n_pixels < 2^32.
 *
 * iamx_colour_accumulate: sum DEV uint32 [n_values] += frames[0] + ... + frames[n_frames-1];
 *   frames is a HOST list of 1 .. iamx_colour_accumulate_max_frames() (8) DEV pointers: the sum is
 *   read and written once per launch, whatever the number of frames.
 *
 * iamx_colour_mean: avg[i] = uint8(trunc(float32(sum[i]) / float32(count))), the division rounded
 *   once: numpy's (sum / count).astype('uint8') on the float32 sum of 99-vignette.py:63,69, which
 *   is exact while 255 * count < 2^24.  count above 65 793 is IAMX_EINVAL.
 *
 * iamx_colour_moments: with r = double(float(sqrt(dx*dx + dy*dy))) about (cu, cv) (the reference
 *   keeps its radii in a float32 table), *radius (HOST) = R = the largest r of the image (a corner)
 *   and s = r / R, out DEV double [3][8] = per channel { sum s^8, s^6, s^4, s^2, n, s^4 v, s^2 v, v }:
 *   the normal equations of v ~ a' s^4 + b' s^2 + c (a = a'/R^4, b = b'/R^2).  partials DEV double
 *   [iamx_colour_moments_workspace_doubles()].  A fixed grid, a fixed tree per workgroup and the
 *   partials added in index order: two runs give the same bits.  No floating-point atomics.
 *
 * iamx_colour_fit_mask: out[y][x][ch] = dither(a r^4 + b r^2 + c) with r = sqrt(dx*dx + dy*dy) in
 *   doubles and the polynomial evaluated as a*r*r*r*r + b*r*r + c; coef HOST double [3][3] = per
 *   channel a, b, c.  dither(x) = trunc(x), plus one with probability x - trunc(x); the uniform number
 *   is a hash of (seed, 3*(y*width + x) + ch): no state, the same seed gives the same mask.  A
 *   polynomial that leaves [0, 255] inside the image is IAMX_EINVAL (checked on the host at the
 *   nearest and the farthest pixel and at the vertex), as the reference's uint8 assignment raises.
 *
 * iamx_colour_mask_finish: per channel m = 255 - v, m -= min(m) (99-vignette.py:142-149), i.e.
 *   out = max(v) - v.  chan_max DEV uint32 [3] is scratch.  out may be img.
 *
 * iamx_colour_lut: out[i] = lut[i % 3][img[i]], lut DEV uint8 [3][256]; with mask (DEV uint8
 *   [n_values], may be null) out[i] = min(255, lut[..] + mask[i]) in the same pass.  out may be img.
 * ------------------------------------------------------------------------------------ */
int iamx_colour_histogram(const uint8_t *img, int64_t n_pixels, uint32_t *hist, void *stream);
int iamx_colour_accumulate_max_frames(void);
int iamx_colour_accumulate(const uint8_t *const *frames, int n_frames, int64_t n_values, uint32_t *sum,
                           void *stream);
int iamx_colour_mean(const uint32_t *sum, int64_t n_values, int count, uint8_t *avg, void *stream);
int iamx_colour_moments_workspace_doubles(void);
int iamx_colour_moments(const uint8_t *img, int height, int width, double cu, double cv, double *radius,
                        double *partials, double *out, void *stream);
int iamx_colour_fit_mask(int height, int width, double cu, double cv, const double *coef, uint64_t seed,
                         uint8_t *out, void *stream);
int iamx_colour_mask_finish(const uint8_t *img, int64_t n_pixels, uint32_t *chan_max, uint8_t *out,
                            void *stream);
int iamx_colour_lut(const uint8_t *img, int64_t n_pixels, const uint8_t *lut, const uint8_t *mask,
                    uint8_t *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Step 5 surface grids -- replace the per-point scipy.interpolate.LinearNDInterpolator calls of
 * scripts/lib/render_panda3d.py:25-78,148-225 (intersect2d / intersect_vectors, with
 * project.projectVectors and project.intersectVectorsWithGroundPlane).  The Delaunay
 * triangulation itself stays scipy.spatial.Delaunay on the host; all pointers are DEV.
 *
 * iamx_surface_pack: simplices [T][3] i32, neighbors [T][3] i32 (-1 at the hull), transform
 *   [T][3][2] f64 as scipy gives them -> records [T] of IAMX_SURFACE_RECORD_BYTES (128-byte
 *   aligned): one step of a walk touches one record.
 *
 * The walk of a query (x, y): in triangle s, c0, c1 = rows 0, 1 of transform[s] applied to
 *   (x, y) - transform[s][2], c2 = 1 - (c0 + c1); smallest c >= -100 DBL_EPSILON: inside, value
 *   c0 z[v0] + c1 z[v1] + c2 z[v2] summed in that order; else step to the neighbour opposite the
 *   smallest c, -1 = outside the hull = NaN.  A walk of more than max_steps records (0: T + 16), a
 *   NaN transform or a NaN query is NOT answered: its flag is set and the caller asks scipy.
 *   seed [G][G] i32: start triangle of the cell (row = y) of bbox = {xmin, ymin, xmax, ymax}
 *   (HOST pointer, 4 doubles), queries outside the box start from the nearest cell.
 *
 * iamx_surface_interp: xy [N][2] -> out [N] f64, flags [N] u8 (1 = not answered), steps [N] i32
 *   (records read; may be null).
 *
 * iamx_surface_grid: one thread per (image, grid vertex).  M [I][9] = body2ned . cam2body . IK,
 *   ned [I][3], avg_ground [I] = -z_avg, uv [n][2] the shared pixel grid.  Ray = unit(M [u, v, 1]),
 *   then intersect2d as written: v[2] <= 0 -> the camera position (IAMX_SURFACE_SKY); first look-up
 *   at the camera position from the seed grid, NaN there -> avg_ground unless no_extrapolate; up to
 *   25 rounds while |p[2] - surface| > 0.01, p recomputed from ned, a NaN inside the loop keeps the
 *   previous surface, every look-up starting where the previous one ended; atan2(-dz, dist) < 30
 *   degrees -> three NaNs (IAMX_SURFACE_HIGH_ANGLE).  A ray with a look-up that was not answered
 *   carries IAMX_SURFACE_FALLBACK and its point is not valid.  ground_mode != 0: no triangulation
 *   (records .. bbox may be null), intersectVectorsWithGroundPlane(ned, ground_m, rays).
 *   pts [I][n][3] f64 NED, rounds [I][n] i32, flags [I][n] u8, steps [I][n] i32 or null.
 * ------------------------------------------------------------------------------------ */
#define IAMX_SURFACE_RECORD_BYTES 128
#define IAMX_SURFACE_MAX_TRIANGLES (1 << 24)
#define IAMX_SURFACE_MAX_SEED_GRID 4096
#define IAMX_SURFACE_SKY 1
#define IAMX_SURFACE_HIGH_ANGLE 2
#define IAMX_SURFACE_FALLBACK 4
int iamx_surface_pack(const int *simplices, const int *neighbors, const double *transform,
                      int num_triangles, void *records, void *stream);
int iamx_surface_interp(const void *records, int num_triangles, const double *values, int num_points,
                        const int *seed, int seed_g, const double *bbox, const double *xy,
                        int64_t num_queries, int max_steps, double *out, uint8_t *flags, int *steps,
                        void *stream);
int iamx_surface_grid(const void *records, int num_triangles, const double *values, int num_points,
                      const int *seed, int seed_g, const double *bbox, const double *M,
                      const double *ned, const double *avg_ground, int num_images, const double *uv,
                      int num_vertices, int no_extrapolate, int ground_mode, double ground_m,
                      int max_steps, double *pts, int *rounds, uint8_t *flags, int *steps,
                      void *stream);

/* ------------------------------------------------------------------------------------
 * Terrain (csrc/terrain.hip) -- the NED elevation grid of scripts/lib/srtm.py:179-254 and its
 * readers: ned_interp (scipy.interpolate.RegularGridInterpolator, linear, bounds_error=False,
 * fill_value=-32768) and interpolate_vector (:277-314).  All pointers are DEV, all arithmetic f64.
 *
 * The terrain: axis_n [rows], axis_e [cols] strictly ascending (np.linspace: not exactly
 *   uniform; the interval is found from a uniform guess corrected against the axis), grid
 *   [rows][cols].  2 <= rows, cols <= IAMX_TERRAIN_MAX_AXIS.
 *
 * iamx_terrain_heights: pts [N][2] (n, e) -> z [N].  A NaN coordinate -> NaN; outside
 *   [axis[0], axis[-1]] on either axis -> -32768; else with a[i] <= x < a[i+1] (last interval
 *   closed), t = (x - a[i]) / (a[i+1] - a[i]):
 *   g00 (1-tn)(1-te) + g01 (1-tn) te + g10 tn (1-te) + g11 tn te, multiplied and summed left to right.
 *
 * iamx_terrain_rays: one thread per (image, ray).  M [I][9], ned [I][3], uv [n][2]; ray =
 *   unit(M [u, v, 1]) (render_panda3d.unit_rays).  iamx_terrain_rays_vec takes ready vectors
 *   v [I][n][3] instead.  Then interpolate_vector as written: v[2] <= 0 -> the camera position
 *   (IAMX_TERRAIN_SKY); first look-up under the camera, 0.0 where it is NaN or not above -32768;
 *   while error > 0.01 and count < 25: d = -(ned[2] + ground), p = ned + v (d / v[2]) with
 *   p[2] = ned[2] + d, look-up at p keeps the previous ground where it is NaN or not above
 *   -32768, error = |p[2] + ground|.  IAMX_TERRAIN_CAPPED: 25 rounds and the error still above
 *   0.01; IAMX_TERRAIN_LEFT_GRID: a look-up of the ray was outside the grid.
 *   pts [I][n][3] f64 NED, iters [I][n] u8, flags [I][n] u8.
 * ------------------------------------------------------------------------------------ */
#define IAMX_TERRAIN_MAX_AXIS 32768
#define IAMX_TERRAIN_SKY 1
#define IAMX_TERRAIN_CAPPED 2
#define IAMX_TERRAIN_LEFT_GRID 4
int iamx_terrain_heights(const double *axis_n, int rows, const double *axis_e, int cols,
                         const double *grid, const double *pts, int64_t num_points, double *z,
                         void *stream);
int iamx_terrain_rays(const double *axis_n, int rows, const double *axis_e, int cols,
                      const double *grid, const double *M, const double *ned, int num_images,
                      const double *uv, int num_rays, double *pts, uint8_t *iters, uint8_t *flags,
                      void *stream);
int iamx_terrain_rays_vec(const double *axis_n, int rows, const double *axis_e, int cols,
                          const double *grid, const double *v, const double *ned, int num_images,
                          int num_rays, double *pts, uint8_t *iters, uint8_t *flags, void *stream);

/* ------------------------------------------------------------------------------------
 * K1: SIFT detect + describe -- replaces cv2.SIFT_create().detectAndCompute(scaled, None)
 *   scripts/lib/image.py:235-237,324 (OpenCV defaults: 3 layers/octave, sigma 1.6, image
 *   doubled, contrastThreshold 0.04, edgeThreshold 10, no feature cap).
 *   image      DEV [height][width][channels] uint8, channels = 3 (BGR) or 1 (gray)
 *   workspace  DEV, iamx_sift_workspace_bytes(height, width) bytes (pyramids + candidates)
 *   kp         DEV [cap][8] float32: x, y (input-image px), size, angle (deg), response,
 *              packed octave (int32 bit pattern, cv2.KeyPoint.octave), 2 internal words
 *   desc       DEV [cap][128] uint8 (what cv2 returns as float32 0..255)
 *   n_out      DEV [1] int32: keypoints found (may exceed cap; only cap are stored)
 * Keypoints are appended in no particular order and still hold duplicates; iamx_sift_sort is the
 * rest of detectAndCompute: KeyPointsFilter::removeDuplicatedSorted (duplicates dropped, OpenCV's
 * output order).  Behind the float32 pyramid the arithmetic follows OpenCV's sift.simd.hpp scalar
 * code in float32 (adjustLocalExtrema with Matx33f::solve, calcOrientationHist,
 * calcSIFTDescriptor, hal::fastAtan2); oracle/sift_oracle.py and DESIGN.md section 2 state the
 * four departures: (a) - (c) in the arithmetic, (d) the 33-tap limit, which is this:
 *   sigma      a Gaussian kernel keeps at most 33 taps: its radius is capped at 16 and the kept taps
 *              are renormalised.  The levels are OpenCV's Gaussians (round(8 s + 1) | 1 taps for a
 *              blur of s) only while every layer's round(8 sigma_i + 1) | 1 <= 33, i.e. for
 *              sigma <= 2.10 (the widest layer blur is 1.9312 sigma); above that the upper layers
 *              of every octave are truncated Gaussians, which cv2 would not produce.
 * ------------------------------------------------------------------------------------ */
int64_t iamx_sift_workspace_bytes(int height, int width);
int iamx_sift_detect(const uint8_t *image, int height, int width, int channels,
                     float contrast_threshold, float edge_threshold, float sigma,
                     void *workspace, int64_t workspace_bytes, float *kp, uint8_t *desc, int cap,
                     int32_t *n_out, void *stream);

/* Where a pyramid level lives inside the workspace after iamx_sift_detect (tests / diagnosis):
 * kind 0 = Gaussian level index 0..5 of `octave` (0 = the doubled image); float32
 * [level_h][level_w] at workspace + byte_offset.  Other kinds fail: the DoG levels are not
 * stored (level i + 1 minus level i is taken where the scan and the sub-pixel fit need it). */
int iamx_sift_pyramid_level(int height, int width, int octave, int kind, int index,
                            int64_t *byte_offset, int *level_h, int *level_w, int *n_octaves);

/* KeyPointsFilter::removeDuplicatedSorted of detectAndCompute (OpenCV features2d/keypoint.cpp;
 * cv2.SIFT.detectAndCompute at scripts/lib/image.py:324 returns its result) on the lists
 * iamx_sift_detect appended: sort by KeyPoint12_LessThan -- x, y ascending, size descending, angle
 * ascending, response descending, octave descending -- and drop every keypoint equal to its
 * predecessor in (x, y, size, angle).  order 1 = that order (what cv2 returns); order 0 = the
 * pyramid-local (octave, layer, y, x, angle) order with the same duplicates dropped.
 * n_out DEV [1] as written by iamx_sift_detect; width, height: the detect image's size in pixels;
 * out_kp DEV [cap][8], out_desc DEV [cap][128] (rows [0, n_sorted)); n_sorted DEV [1] int32 =
 * rows kept; workspace DEV iamx_sift_sort_workspace_bytes(cap) bytes. */
int64_t iamx_sift_sort_workspace_bytes(int cap);
int iamx_sift_sort(const float *kp, const uint8_t *desc, const int32_t *n_out, int cap, int order,
                   int width, int height, void *workspace, int64_t workspace_bytes, float *out_kp,
                   uint8_t *out_desc, int32_t *n_sorted, void *stream);

/* ------------------------------------------------------------------------------------
 * Image ingest: split JPEG decoder (csrc/jpeg.hip) in place of cv2.imread(file, ANYCOLOR |
 * ANYDEPTH | IGNORE_ORIENTATION) of scripts/lib/image.py:99-104.  The host does the Huffman
 * decode (serial by nature), the device dequantisation + the libjpeg "islow" integer IDCT +
 * fancy chroma upsampling + YCbCr -> BGR: integer arithmetic throughout, pixels bit-identical to
 * libjpeg-turbo's (what OpenCV and Pillow decode with).  8-bit baseline / extended-sequential
 * Huffman files with one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0; anything else
 * returns IAMX_EUNSUPPORTED (the caller decodes such a file the host way).
 *   iamx_jpeg_info: HOST.  info [16] int32: width, height, components, max h / v sampling,
 *     blocks_w / blocks_h of components 0..2 (8x8 blocks, padded to whole MCUs), [11] total
 *     blocks, [12] restart interval.
 *   iamx_jpeg_decode_coefficients: HOST, no device involved, thread safe.  coef HOST
 *     [coef_blocks >= info[11]][64] int16: the quantised coefficients of every block in natural
 *     (row major) order, components back to back, blocks of a component in raster order;
 *     quant HOST [3][64] uint16: the components' quantisation tables in natural order.
 *   iamx_jpeg_reconstruct: coef / quant DEV (as written above), info HOST, workspace DEV
 *     iamx_jpeg_workspace_bytes(info) bytes (the component planes), bgr DEV [height][width][3].
 * ------------------------------------------------------------------------------------ */
int iamx_jpeg_info(const uint8_t *data, int64_t len, int32_t *info);
int iamx_jpeg_decode_coefficients(const uint8_t *data, int64_t len, int16_t *coef,
                                  int64_t coef_blocks, uint16_t *quant);
int64_t iamx_jpeg_workspace_bytes(const int32_t *info);
int iamx_jpeg_reconstruct(const int16_t *coef, const uint16_t *quant, const int32_t *info,
                          void *workspace, int64_t workspace_bytes, uint8_t *bgr, void *stream);

/* Entropy decoding on the device (csrc/jpeg_entropy.hip, method in csrc/jpeg_entropy.h): the
 * Huffman-coded scan of the same class of file becomes the same coefficients, in device memory,
 * without the host decode and without the upload of blocks x 128 bytes -- only the file goes up.
 * The scan is decoded as sub-sequences of 128 bytes or more (two average MCUs), one lane each, that
 * fall into step with the true decode (self-synchronisation); the result is exact or refused,
 * never approximately right.
 *   iamx_jpeg_entropy_prepare: HOST (markers and tables only, microseconds).  info [16] and quant
 *     [3][64] as iamx_jpeg_info / iamx_jpeg_decode_coefficients fill them; header HOST
 *     [header_bytes >= iamx_jpeg_entropy_header_bytes()]: tables in look-up form, geometry, offset
 *     and length of the scan.  Errors are the host parser's (IAMX_EUNSUPPORTED / IAMX_EINVAL);
 *     additionally IAMX_EUNSUPPORTED for a scan above 128 MiB, for a file without entropy-coded
 *     data and for tables that hold a code of all ones in a file with restart markers.  The scan
 *     the header describes ends at the first marker that is not a restart marker of the file, as
 *     it does for the host half: bytes behind EOI (previews, maker blobs) are never decoded.
 *   iamx_jpeg_entropy_workspace_bytes(header HOST): bytes of DEV workspace one call needs (0 for
 *     a pointer that is not such a header).  The workspace belongs to one call at a time.
 *   iamx_jpeg_entropy_decode: asynchronous on `stream`; no allocation, no synchronisation.
 *     data DEV: the whole file, 16-byte aligned, data_bytes >= its length rounded up to 16 (the
 *     padding is loaded, never used); header HOST and d_header DEV (a 16-byte aligned copy of
 *     it); workspace DEV, 16-byte aligned; coef DEV [coef_blocks >= info[11]][64] int16, written
 *     as iamx_jpeg_decode_coefficients writes it; status DEV int32 [4], valid once the stream
 *     has passed the call: [0] one of IAMX_JPEG_*, [1] the synchronisation passes it took, [2] the
 *     sub-sequences those passes decoded, all together (each reads its share of the scan once;
 *     the write pass reads every one once more), [3] 0.
 *     Bad arguments return IAMX_EINVAL before anything touches the device.  The call trusts what
 *     it cannot check from the host: `header` must be what iamx_jpeg_entropy_prepare wrote,
 *     unchanged (its geometry is validated, the six tables are not), and d_header a copy of it.
 *     Every lane makes at most 8 x sub-sequence bytes + 64 decode steps, whatever frame size the
 *     file claims.
 * status[0]:
 *   IAMX_JPEG_SYNCED      every sub-sequence start was verified, coef holds the host half's values
 *   IAMX_JPEG_NOT_SYNCED  no fixed point inside the pass bound (flat images never synchronise, a flat
 *                         stretch of more than 47 sub-sequences inside an image does not either): coef
 *                         is zero, decode this file with iamx_jpeg_decode_coefficients
 *   IAMX_JPEG_DAMAGED     verified, but the data ended before the last block (truncation, a stray
 *                         marker such as FF FF Dn) or a restart marker stood inside an MCU: coef
 *                         holds what was decoded and zeros behind it; the host half, which goes on
 *                         with zero bits, is the reference for such a file */
#define IAMX_JPEG_PENDING     0
#define IAMX_JPEG_SYNCED      1
#define IAMX_JPEG_NOT_SYNCED  2
#define IAMX_JPEG_DAMAGED     3
int64_t iamx_jpeg_entropy_header_bytes(void);
int iamx_jpeg_entropy_prepare(const uint8_t *data, int64_t len, int32_t *info, uint16_t *quant,
                              void *header, int64_t header_bytes);
int64_t iamx_jpeg_entropy_workspace_bytes(const void *header);
int iamx_jpeg_entropy_decode(const uint8_t *data, int64_t data_bytes, const void *header,
                             const void *d_header, void *workspace, int64_t workspace_bytes,
                             int16_t *coef, int64_t coef_blocks, int32_t *status, void *stream);

/* The reference's descriptor cache file (gzip of np.save(float32 [N, 128]),
 * scripts/lib/image.py:205-217) written straight from the detector's uint8 descriptors: HOST,
 * no device involved, thread safe.  out receives ONE gzip member whose payload is `header` (the
 * .npy header) followed by the little-endian float32 values of `values`; any gzip reader gets the
 * bytes np.save would have written (a dynamic-Huffman DEFLATE block of literals built from the
 * histogram of the 256 possible values: ~25 ms per 50 k-keypoint frame instead of ~0.5 s of
 * zlib).  Returns the member's size in bytes (out_cap >= iamx_gzip_f32_from_u8_bound(...)) or a
 * negative error code. */
int64_t iamx_gzip_f32_from_u8_bound(int64_t n_header, int64_t n_values);
int64_t iamx_gzip_f32_from_u8(const uint8_t *header, int64_t n_header, const uint8_t *values,
                              int64_t n_values, uint8_t *out, int64_t out_cap);

/* The other cache-file byte work of Image.save_features / save_descriptors / detect_features
 * (scripts/lib/image.py:187-217, 324-346), HOST only, one call each so that no interpreter lock
 * is held or handed around while the bytes are produced (threads are created inside):
 *   iamx_gzip_members   gzip.open(..., compresslevel=level).write(...) as a multi-member gzip
 *                       stream (members of <= member_bytes of input, compressed in parallel with
 *                       zlib at `level`, `strategy` 0 default .. 4 fixed as in zlib.h); bufs / lens: the buffers that follow each other (an .npy header and
 *                       the array's own memory, or one pickle).  Returns bytes written
 *                       (out_cap >= iamx_gzip_members_bound(total, members)) or a negative code.
 *   iamx_u8_to_f32      des_list = float32 of the detector's uint8 descriptors.
 *   iamx_feat_records   the .feat pickle's records "( G x G y TUPLE2 G size G angle G response
 *                       J octave J class_id t" (58 bytes per keypoint) from the columns. */
int64_t iamx_gzip_members_bound(int64_t total_bytes, int64_t n_members);
int64_t iamx_gzip_members(const uint8_t *const *bufs, const int64_t *lens, int n_bufs,
                          int64_t member_bytes, int level, int strategy, int threads, uint8_t *out,
                          int64_t out_cap);
/* iamx_gzip_records -- HOST.  iamx_gzip_members for streams of fixed-width records (the .feat
 * pickle of scripts/lib/image.py:192-203: 58 bytes per keypoint): a DEFLATE encoder that only
 * looks for matches at distance record_bytes (one compare pass, dynamic Huffman code, no hash
 * chains) -- valid gzip members, the same payload for every reader, smaller than zlib's level 4
 * output on such streams and several times faster.  out_cap >= iamx_gzip_records_bound(total
 * input bytes, number of members). */
int64_t iamx_gzip_records_bound(int64_t total, int64_t n_members);
int64_t iamx_gzip_records(const uint8_t *const *bufs, const int64_t *lens, int n_bufs,
                          int64_t member_bytes, int record_bytes, int threads, uint8_t *out,
                          int64_t out_cap);
int iamx_u8_to_f32(const uint8_t *src, float *dst, int64_t n, int threads);
/* the other way for a whole survey: the float32 des_list of n images (scripts/lib/image.py:324,
 * integer valued) -> uint8 back to back in dst (HOST), threads of its own; srcs HOST [n] pointers,
 * counts HOST [n] elements per image.  Feeds ONE upload + the batched pack kernels. */
int iamx_f32_to_u8_many(const float *const *srcs, const int64_t *counts, int n, uint8_t *dst,
                        int threads);
/* n host byte blocks (counts[i] bytes at srcs[i]) copied back to back into dst by `threads` threads:
 * the uint8 descriptor arrays of a group of images into one page-locked staging buffer. */
int iamx_u8_gather_many(const uint8_t *const *srcs, const int64_t *counts, int n, uint8_t *dst,
                        int threads);
int iamx_feat_records(const float *x, const float *y, const float *size, const float *angle,
                      const float *response, const int32_t *octave, const int32_t *class_id,
                      int64_t n, uint8_t *out);
/* The pair lists of the .match pickles (Image.save_matches, scripts/lib/image.py:222-233): list k =
 * rows [off[k], off[k+1]) of pairs [.][2] as the protocol-2 stream "] ( { ] ( int int e }* e" (no
 * memo entries), an empty list as "]"; out_off [n_lists + 1] receives where each list's bytes start
 * (out_cap >= sum of 3 + 13 * rows).  HOST only.  Returns bytes written or a negative code. */
int64_t iamx_pickle_pair_lists(const int32_t *pairs, const int64_t *off, int64_t n_lists, uint8_t *out,
                               int64_t out_cap, int64_t *out_off);

/* ------------------------------------------------------------------------------------
 * K4: linear algebra on the device-resident block Jacobian (what SciPy's TRF/LSMR does on
 * the sparse matrix the reference gives it: scripts/lib/optimizer.py:491-501,
 * scipy/optimize/_lsq/trf.py:205-400).  n = 7*n_cams + 3*n_pts (+8 with Jk), m = 2*n_obs.
 *   iamx_ba_jv   y[m] = J x
 *   iamx_ba_jtv  out[n] = J^T u            (square = 0)
 *                out[n] = column sums of J.^2 (square != 0; u unused) -- x_scale='jac'
 *     cam_ptr DEV [n_cams+1] int32: observations of camera c are [cam_ptr[c], cam_ptr[c+1])
 *             (the camera-major order of optimizer.py:397-404)
 *     pt_ptr  DEV [n_pts+1], pt_obs DEV [n_obs] int32: observation ids grouped by point
 *     scratch DEV [2048] float64 (only read/written when Jk != NULL)
 *   No atomics: results are bitwise reproducible.
 * ------------------------------------------------------------------------------------ */
int iamx_ba_jv(const double *Jc, const double *Jp, const double *Jk, const int32_t *cam_idx,
               const int32_t *pt_idx, int64_t n_obs, int n_cams, int n_pts, const double *x,
               double *y, void *stream);
int iamx_ba_jtv(const double *Jc, const double *Jp, const double *Jk, const int32_t *cam_ptr,
                const int32_t *pt_ptr, const int32_t *pt_obs, int64_t n_obs, int n_cams,
                int n_pts, const double *u, int square, double *out, double *scratch,
                void *stream);

/* Host-free, matrix-free LSMR (scipy/sparse/linalg/_isolve/lsmr.py) on
 * A = [J diag(d); diag(dreg)], b = [r; 0], no calibration columns.  J is the analytic Jacobian
 * of iamx_ba_residual_jac at (cams, pts, calib); the kernels re-derive an observation's 2x10
 * block from its camera and point instead of reading a stored copy.
 * iamx_ba_lsmr_prepare: once per solve, the tables
 *   ctab DEV [n_cams][32] (rotation, position, quaternion, 1/|q|^2, d of the 7 columns),
 *   ptab DEV [n_pts][6]  (X, d of the 3 columns).
 * iamx_ba_lsmr_iterate: enqueues n_iter (even) iterations, three launches each, no host
 *   synchronisation.  `state` (DEV, iamx_ba_lsmr_state_size() doubles) holds the double-
 *   buffered scalar recurrences, the tolerances and the latched results (layout and
 *   initialisation: imageanalysis_amd/ba_solver.py); once istop is latched the remaining
 *   iterations are no-ops.  u1 [2 n_obs], u2/vt/h/hbar/x [n] DEV work vectors; partials DEV
 *   [iamx_ba_lsmr_partials_size]; xr DEV [4] (sums that cross kernels), tbuf DEV [n] (raw J^T ut1).
 *   pt_idx [n_obs] camera-major; cam_ptr / pt_ptr / pt_obs as for iamx_ba_jtv; slot_cp DEV
 *   [n_obs][2] int32 = (camera, point) of the observation in point-sorted slot e = pt_obs[e].
 *   eprod DEV [n_obs][3] float64 work buffer: the point part of J^T ut' per observation, written
 *   by the forward kernel (which has the observation's geometry and the new ut' in registers) and
 *   summed per point by the adjoint kernel.
 *   Deterministic (fixed reduction trees, no atomics). */
int iamx_ba_lsmr_state_size(void);
int64_t iamx_ba_lsmr_partials_size(int n_cams, int n_pts);
int iamx_ba_lsmr_prepare(const double *cams, const double *pts, const double *d, int n_cams,
                         int n_pts, double *ctab, double *ptab, void *stream);
int iamx_ba_lsmr_iterate(const double *ctab, const double *ptab, const double *calib,
                         const int32_t *pt_idx, const int32_t *cam_ptr, const int32_t *pt_ptr,
                         const int32_t *pt_obs, const int32_t *slot_cp, int64_t n_obs, int n_cams,
                         int n_pts, const double *dreg, double *u1, double *u2, double *vt,
                         double *h, double *hbar, double *x, double *state, double *partials,
                         double *xr, double *tbuf, double *eprod, int n_iter, void *stream);

/* Multi-rank form of the same iteration: observations AND the point part of every n-vector are
 * sharded by point (this rank owns the points [pt_lo, pt_hi) of the internal order and every
 * observation of them); only the camera part (7 n_cams entries) is replicated.  One call per
 * phase; the caller all-reduces (sum, RCCL, same stream) xr[0..2) after phase 0 and
 * tbuf[0 .. 7 n_cams] (7 n_cams + 1 doubles: 157 KB at BASELINE configs[3]) after phase 1.
 *   phase 0: ut', raw camera part of J^T ut1' -> tbuf; xr[0] / xr[1] = this rank's parts of
 *            |ut'|^2 / |x|^2, xr[2] / xr[3] = their replicated camera parts
 *   phase 1: stopping tests of the previous iteration, beta', point part of vt' (rank local),
 *            tbuf[7 n_cams] = its sum of squares
 *   phase 2: camera part of vt' from the reduced tbuf, alpha', plane rotations, h / hbar / x
 * parity = iteration & 1.  xr DEV [4], tbuf DEV [n].  The point entries of x that belong to
 * other ranks are never touched (all-reduce x[7 n_cams ..) once per solve when x started 0).
 * In iamx_ba_lsmr_iterate (single rank) xr is DEV [4] as well. */
int iamx_ba_lsmr_phase(const double *ctab, const double *ptab, const double *calib,
                       const int32_t *pt_idx, const int32_t *cam_ptr, const int32_t *pt_ptr,
                       const int32_t *pt_obs, const int32_t *slot_cp, int64_t n_obs, int n_cams,
                       int n_pts, int pt_lo, int pt_hi, const double *dreg, double *u1, double *u2,
                       double *vt, double *h, double *hbar, double *x, double *state,
                       double *partials, double *xr, double *tbuf, double *eprod, int phase,
                       int parity, void *stream);

/* ------------------------------------------------------------------------------------
 * Normal-equation blocks and the Schur-complement Gauss-Newton step (csrc/ba_schur.hip).
 *
 * iamx_ba_accumulate (the J^T J / J^T r accumulators of BASELINE.json's north star):
 *   one pass over the stored block Jacobian of iamx_ba_residual_jac emits
 *     U  DEV [n_cams][7][7]  = sum over the camera's observations of Jc^T Jc
 *     V  DEV [n_pts][3][3]   = sum over the point's observations of Jp^T Jp
 *     gc DEV [n_cams][7]     = sum Jc^T r,     gp DEV [n_pts][3] = sum Jp^T r
 *   i.e. the block diagonal of J^T J and the gradient J^T r that scipy's TRF derives from the
 *   sparse J the reference gives it (scripts/lib/optimizer.py:142-169, 491-501;
 *   scipy/optimize/_lsq/trf.py:241-247 g = compute_grad(J, f), compute_jac_scale).  diag(U),
 *   diag(V) are the column sums of J.^2 of x_scale='jac'.  The off-diagonal blocks W = Jc^T Jp
 *   (7x3 per observation) are never stored: the solve below applies them from Jc / Jp.
 *   cam_ptr / pt_ptr / pt_obs as for iamx_ba_jtv.  Observations sharded by point over several
 *   ranks: U and gc are partial sums -- all-reduce them (n_cams x 56 doubles, once per outer
 *   iteration); V and gp are complete on the rank that owns the point.  No atomics.
 *
 * The trust-region subproblem  min || [J diag(d); diag(dreg)] p - [r; 0] ||  of trf.py:303-314
 * (which SciPy hands to LSMR: iamx_ba_lsmr_* keeps that form) through its normal equations:
 * points eliminated exactly, the reduced camera system S p_c = b solved by conjugate gradients
 * preconditioned with the inverses of S's 7x7 diagonal blocks, then p_p back-substituted.
 *   iamx_ba_schur_prepare: Y DEV [n_pts][6] = (D_p V D_p + Dreg_p^2)^-1 (upper triangle),
 *     yg DEV [n_pts][3] = Y D_p gp, zp DEV [n_pts][3] work, sraw DEV [n_cams][35] = the packed
 *     upper triangle of this rank's part of S_cc before regularisation (28) + its part of b (7)
 *     -- all-reduce sraw over ranks.  d, dreg DEV [n] (n = 7 n_cams + 3 n_pts).
 *   iamx_ba_schur_factor: one workgroup: M_c = (S_cc + Dreg_c^2)^-1 -> minv DEV [n_cams][28]
 *     (Cholesky; a block that is not positive definite falls back to its diagonal), x = 0,
 *     r = b, z = M r, p = z, y = d_c .* p, state (DEV, iamx_ba_schur_state_size() doubles = two
 *     buffers of 16; buffer 0 is the start:
 *     [0] r.z, [1] initial r.z, [2] iterations done, [3] stop: 0 running / 1 sqrt(r.z / r0.z0) <=
 *     eta / 2 max_iter reached / 3 breakdown / 4 the decrease of the quadratic model
 *     Q(x) = x.Sx/2 - b.x has levelled off: i (Q_{i-1} - Q_i) <= qtol |Q_i|, [4] eta,
 *     [5] max_iter, [6] alpha, [7] beta, [8] p.Sp, [9] -Q, [10] qtol)
 *   iamx_ba_schur_iterate: n_iter iterations, five launches each, no host synchronisation;
 *     a latched stop turns everything enqueued behind it into no-ops.  The state block holds
 *     two buffers: iteration i (first_iter = the number of iterations enqueued since
 *     iamx_ba_schur_factor) reads buffer i & 1 and writes the other; after k iterations the
 *     current scalars are in buffer k & 1.  phase = -1: whole iterations (one rank); several
 *     ranks: phase 0 = the three passes of q = S y over this rank's observations -> qraw DEV
 *     [n_cams][7], all-reduce qraw, then phase 1 = the update (scalars replicated on every
 *     rank).  t DEV [2 n_obs], part DEV [2 n_cams] (partials of the two inner products),
 *     x r z p y DEV [7 n_cams].
 *   iamx_ba_schur_finish: step DEV [n] = (x, Y D_p (gp - W^T x)) in the scaled variables of the
 *     subproblem; the point entries outside [pt_lo, pt_hi) are written as 0 (several ranks:
 *     all-reduce the point part once).
 * ------------------------------------------------------------------------------------ */
int iamx_ba_accumulate(const double *Jc, const double *Jp, const double *r, const int32_t *cam_ptr,
                       const int32_t *pt_ptr, const int32_t *pt_obs, int64_t n_obs, int n_cams,
                       int n_pts, double *U, double *V, double *gc, double *gp, void *stream);
/* out DEV [7 n_cams + 3 n_pts] = (diag U, diag V): the column sums of J.^2 */
int iamx_ba_block_diag(const double *U, const double *V, int n_cams, int n_pts, double *out,
                       void *stream);
int iamx_ba_schur_state_size(void);
/* optimize_calib='global' (scripts/lib/optimizer.py:142-169,181-189: 8 calibration columns that
 * every observation shares; `process.py --cam-calibration`, scripts/process.py:384): pass Jk DEV
 * [n_obs][2][8] (iamx_ba_residual_jac) to all four calls for the BORDERED form -- the calibration
 * block joins the camera side of the reduced system as one more block of 8 parameters, with the
 * inverse of its own normal-equation block (D_k sum Jk^T Jk D_k + Dreg_k^2) as preconditioner.
 * Then n = 7 n_cams + 3 n_pts + 8 (calibration entries of d / dreg / step behind the points),
 * x r z p y qraw DEV [7 n_cams + 8], minv DEV [28 n_cams + 36], part DEV [2 (n_cams + 1)], sraw DEV
 * [35 n_cams + 44] (all-reduce all of it), ckpart DEV [n_cams][44] scratch; several ranks
 * all-reduce qraw [7 n_cams + 8] per iteration.  Jk = NULL: cameras and points only, sizes as
 * documented above, ckpart unused. */
int iamx_ba_schur_prepare(const double *Jc, const double *Jp, const double *Jk, const double *r,
                          const int32_t *cam_ptr, const int32_t *pt_idx, int64_t n_obs, int n_cams,
                          int n_pts, const double *V, const double *gp, const double *d,
                          const double *dreg, double *Y, double *yg, double *zp, double *sraw,
                          double *ckpart, void *stream);
int iamx_ba_schur_factor(const double *sraw, const double *d, const double *dreg, int n_cams,
                         int n_pts, int with_calib, double eta, double qtol, int max_iter,
                         double *minv, double *x, double *r, double *z, double *p, double *y,
                         double *state, void *stream);
int iamx_ba_schur_iterate(const double *Jc, const double *Jp, const double *Jk,
                          const int32_t *cam_idx, const int32_t *pt_idx, const int32_t *cam_ptr,
                          const int32_t *pt_ptr, const int32_t *pt_obs, int64_t n_obs, int n_cams,
                          int n_pts, const double *d, const double *dreg, const double *Y,
                          const double *minv, double *t, double *zp, double *qraw, double *part,
                          double *ckpart, double *x, double *r, double *z, double *p, double *y,
                          double *state, int first_iter, int n_iter, int phase, void *stream);
int iamx_ba_schur_finish(const double *Jc, const double *Jp, const double *Jk,
                         const int32_t *cam_idx, const int32_t *pt_ptr, const int32_t *pt_obs,
                         int64_t n_obs, int n_cams, int n_pts, int pt_lo, int pt_hi, const double *d,
                         const double *Y, const double *yg, const double *x, double *y, double *t,
                         double *step, void *stream);

/* ------------------------------------------------------------------------------------
 * Robust loss functions of the bundle adjustment (csrc/ba_robust.hip) -- the loss= / f_scale= of
 * scipy.optimize.least_squares (construct_loss_function, scale_for_robust_loss_function), per
 * scalar residual component f with C = f_scale, z = (f / C)^2:
 *   iamx_ba_robust_cost: out[0] = sum rho(z) over r DEV [m] (cost = 0.5 C^2 out[0]); fixed grid and
 *     fixed reduction tree, no atomics: two calls give the same bits.  scratch DEV [256] float64.
 *   iamx_ba_robust_scale: in place, from the unscaled residuals of r DEV [n_obs][2]:
 *     J_scale = max(rho' + 2 rho'' z, 2^-52);  f *= rho' / sqrt(J_scale);  the row of f in Jc DEV
 *     [n_obs][2][7], Jp DEV [n_obs][2][3] and Jk DEV [n_obs][2][8] (may be NULL) *= sqrt(J_scale).
 *     All four 16-byte aligned (any n_obs: an observation owns an even number of doubles in each).
 * loss is one of IAMX_LOSS_HUBER .. IAMX_LOSS_ARCTAN (IAMX_LOSS_LINEAR needs neither call and is
 * refused); f_scale finite and > 0.  Argument checks need no GPU.
 * ------------------------------------------------------------------------------------ */
enum { IAMX_LOSS_LINEAR = 0, IAMX_LOSS_HUBER = 1, IAMX_LOSS_SOFT_L1 = 2, IAMX_LOSS_CAUCHY = 3,
       IAMX_LOSS_ARCTAN = 4 };
int iamx_ba_robust_cost(const double *r, int64_t m, int loss, double f_scale, double *out,
                        double *scratch, void *stream);
int iamx_ba_robust_scale(double *r, double *Jc, double *Jp, double *Jk, int64_t n_obs, int loss,
                         double f_scale, void *stream);

/* ------------------------------------------------------------------------------------
 * Collectives of the hot path for callers that are not python: RCCL over
 * xGMI, bound at run time (a process that already holds an RCCL -- torch bundles one -- re-uses
 * it).  The python layer does the same two exchanges through torch.distributed.
 *   iamx_comm_unique_id: HOST id128 [128 bytes], created by one rank and handed to the others by
 *     whatever channel the caller has (file, MPI, torch store)
 *   iamx_comm_init: one communicator per process / GPU (the current HIP device); *comm out
 *   iamx_comm_allgather: rank r contributes bytes_per_rank bytes at `send`; recv DEV
 *     [n_ranks * bytes_per_rank]; in place when send == recv + rank * bytes_per_rank -- the packed
 *     descriptor store of the images a rank detected (iamx_desc_pack_* / iamx_desc3_pack_*) in
 *     front of the pair-sharded matching: one large transfer per buffer, never per image
 *   iamx_comm_allreduce_f64: in-place sum -- xr[0..2) and tbuf[0 .. 7 n_cams] between the phases
 *     of iamx_ba_lsmr_phase, the gradient / column norms once per outer iteration
 * All enqueue on `stream`; errors come back as IAMX_ELAUNCH with RCCL's message.
 * ------------------------------------------------------------------------------------ */
int iamx_comm_unique_id(void *id128);
int iamx_comm_init(int n_ranks, int rank, const void *id128, void **comm);
int iamx_comm_destroy(void *comm);
int iamx_comm_allgather(void *comm, const void *send, void *recv, int64_t bytes_per_rank,
                        void *stream);
int iamx_comm_allreduce_f64(void *comm, double *buf, int64_t n, void *stream);

/* float64 vector kernels used by the device LSMR (scipy/sparse/linalg/_isolve/lsmr.py):
 *   axpby: y = a*x + b*y (b == 0 ignores y's old content)
 *   mul2:  out = a.*b (+ c.*d when c != NULL)
 *   dot:   out[0] = sum x.*y, fixed reduction tree (scratch: DEV [256] float64)
 *   lsmr_update: hbar = h + c_hbar*hbar; x += c_x*hbar; h = v + c_h*h */
int iamx_vec_axpby(int64_t n, double a, const double *x, double b, double *y, void *stream);
int iamx_vec_mul2(int64_t n, const double *a, const double *b, const double *c, const double *d,
                  double *out, void *stream);
int iamx_vec_dot(int64_t n, const double *x, const double *y, double *out, double *scratch,
                 void *stream);
int iamx_vec_lsmr_update(int64_t n, double *h, double *hbar, double *x, const double *v,
                         double c_hbar, double c_x, double c_h, void *stream);

/* n-vector kernels of the trust-region-reflective outer loop (csrc/trf_vec.hip), float64, all
 * pointers DEV unless noted.  They restate the O(n) helpers of scipy.optimize.least_squares
 * (method='trf'), which the reference calls at scripts/lib/optimizer.py:352-399:
 *   lincomb: out = a*x + b*y + c*z (y, z may be NULL);  mul: out = s*x.*y (y NULL: s*x)
 *   gather:  out[i] = x[idx[i]] (idx DEV int64 [n]; out must not alias x) -- the private point
 *            order of the device problem <-> the reference's parameter order
 *   sqrt_shift: out = sqrt(x + shift)
 *   dots: out[i] = sum a[i].*b[i] (.*w[i] when w and w[i] are not NULL), 1 <= k <= 8; a, b, w are
 *         HOST arrays of k device pointers; scratch: DEV [iamx_vec_scratch_doubles()] float64
 *   absmax_prod: out[0] = max |x.*y| (y NULL: max |x|), NaN if any product is
 *   trf_cl_scaling:  _lsq/common.py CL_scaling_vector -> v, dv
 *   trf_scale:       trf.py trf_bounds: v[dv != 0] *= scale_inv; d = sqrt(v)/scale_inv;
 *                    diag_h = g.*dv./scale_inv; g_h = d.*g   (v_out may be NULL)
 *   trf_jac_scale:   common.py compute_jac_scale from the column sums of J.^2
 *   trf_step_to_bound: common.py step_size_to_bound -> out[0] = min step
 *   trf_reflect:     its `hits` (equal(steps, min_step) * sign(s)) and r_h = p_h with the hit
 *                    components negated (either output may be NULL)
 *   trf_count_outside: out[0] = number of components of x (+ p) outside [lb, ub] (in_bounds)
 *   trf_strictly_feasible: common.py make_strictly_feasible(x (+ step), lb, ub, rstep=0)
 *   trf_active:      common.py find_active_constraints(x, lb, ub, rtol > 0) as -1 / 0 / +1 */
int iamx_vec_lincomb(int64_t n, double a, const double *x, double b, const double *y, double c,
                     const double *z, double *out, void *stream);
int iamx_vec_mul(int64_t n, double s, const double *x, const double *y, double *out, void *stream);
int iamx_vec_gather(int64_t n, const double *x, const int64_t *idx, double *out, void *stream);
int iamx_vec_sqrt_shift(int64_t n, const double *x, double shift, double *out, void *stream);
int iamx_vec_scratch_doubles(void);
int iamx_vec_dots(int64_t n, int k, const double *const *a, const double *const *b,
                  const double *const *w, double *out, double *scratch, void *stream);
int iamx_vec_absmax_prod(int64_t n, const double *x, const double *y, double *out, double *scratch,
                         void *stream);
int iamx_trf_cl_scaling(int64_t n, const double *x, const double *g, const double *lb,
                        const double *ub, double *v, double *dv, void *stream);
int iamx_trf_scale(int64_t n, const double *v, const double *dv, const double *g,
                   const double *scale_inv, double *v_out, double *d, double *diag_h, double *g_h,
                   void *stream);
int iamx_trf_jac_scale(int64_t n, const double *colsq, double *scale_inv, int first, void *stream);
int iamx_trf_step_to_bound(int64_t n, const double *x, const double *s, const double *lb,
                           const double *ub, double *out, double *scratch, void *stream);
int iamx_trf_reflect(int64_t n, const double *x, const double *s, const double *lb, const double *ub,
                     double min_step, const double *p_h, double *r_h, double *hits, void *stream);
int iamx_trf_count_outside(int64_t n, const double *x, const double *p, const double *lb,
                           const double *ub, double *out, double *scratch, void *stream);
int iamx_trf_strictly_feasible(int64_t n, const double *x, const double *step, const double *lb,
                               const double *ub, double *out, void *stream);
int iamx_trf_active(int64_t n, const double *x, const double *lb, const double *ub, double rtol,
                    double *active, void *stream);
/* make_strictly_feasible(x, lb, ub, rstep) for rstep > 0: the start point of trf_bounds
 * (scipy/optimize/_lsq/trf.py:214 through common.py:440) */
int iamx_trf_feasible_start(int64_t n, const double *x, const double *lb, const double *ub, double rstep,
                            double *out, void *stream);
/* out = x * scale_inv / sqrt(v') with v' = v * scale_inv where dv != 0: the vector whose norm is the
 * first trust-region radius (trf.py:243-246) */
int iamx_trf_scaled_start(int64_t n, const double *x, const double *scale_inv, const double *v,
                          const double *dv, double *out, void *stream);

/* ------------------------------------------------------------------------------------
 * Chain geometry between optimiser passes -- scripts/3c-match-triangulation.py (--method
 * triangulate), scripts/4b-colocated-feats.py and lib/project.py:257-296 (undistort_uvlist,
 * undistort_image_keypoints).  One thread per point / per chain, f64 in stored order, every product
 * and sum rounded on its own.  K4 = {fx, fy, cx, cy} and dist5 = {k1, k2, p1, p2, k3} are HOST
 * pointers; everything else is DEV.  Null and size checks need no GPU; n == 0 returns 0 without a
 * launch.
 *
 * iamx_undistort_points: src [n][2] f32 -> dst [n][2] f32, cv2.undistortPoints(src, K, dist, P=K)
 *   with OpenCV's default criteria as published: x = (u-cx)/fx, y = (v-cy)/fy, five rounds of
 *   r2 = x*x + y*y; icdist = 1/(1 + ((k3*r2 + k2)*r2 + k1)*r2); dx = 2*p1*x*y + p2*(r2 + 2*x*x);
 *   dy = p1*(r2 + 2*y*y) + 2*p2*x*y; x = (x0 - dx)*icdist; y = (y0 - dy)*icdist (icdist < 0: x0, y0
 *   and stop); out = x*fx + cx, y*fy + cy rounded to f32.  Pinned bit for bit to the numpy
 *   restatement tests/undistort_restatement.py; parity with cv2 itself is UNPINNED (cv2 is not
 *   available to the tests), as for CLAHE and the resizes.
 *
 * The chain arrays are match_cleanup.Chains': ptr [n_chains + 1] i64, img [total] i32, uv [total][2]
 * f64, group [n_chains] i32, ned [n_chains][3] f64.  pos [n_images][3] camera positions, in_group
 * [n_images] u8.  A chain is looked at when group[c] == group_index.  An image index outside
 * [0, n_images) in such a chain: IAMX_CHAIN_BAD_IMAGE, nothing is read through it, nothing written.
 *
 * iamx_chain_triangulate: chains with >= 2 members in the group; per such member, in stored order:
 *   uv -> f32 -> undistort (as above) -> f32, v = unit(unit(M [u, v, 1])) with M [n_images][9] =
 *   body2ned . cam2body . inv(K) row major, r += I - v v^T, q += (I - v v^T) pos; r x = q by LU with
 *   partial pivoting (lib/line_solver.py ls_lines_intersection), x -> ned[c].  status [n_chains]:
 *   IAMX_CHAIN_UNTOUCHED / _WRITTEN / _WRITTEN_BELOW (x[2] > 0, the reference's "WHOA!") /
 *   _SINGULAR (zero pivot, ned[c] kept) / _BAD_IMAGE.
 *
 * iamx_chain_pair_angles: members i < j both in the group: v1 = ned[c] - pos[i], v2 = ned[c] - pos[j],
 *   tmp = v1.v2 / (|v1| |v2|), angle = acos(min(tmp, 1)) in degrees, tmp < -1 -> 0 (the reference's
 *   except path), NaN never counts; angle < min_angle_deg: count[i] += 1.  count [total] i32 (every
 *   member of every chain is written), total [1] i64 = sum of count, status [n_chains]:
 *   IAMX_CHAIN_UNTOUCHED / _WRITTEN (scanned) / _BAD_IMAGE.
 * ------------------------------------------------------------------------------------ */
#define IAMX_CHAIN_UNTOUCHED 0
#define IAMX_CHAIN_WRITTEN 1
#define IAMX_CHAIN_WRITTEN_BELOW 2
#define IAMX_CHAIN_SINGULAR 3
#define IAMX_CHAIN_BAD_IMAGE 4
int iamx_undistort_points(const float *src, int64_t n, const double *K4, const double *dist5,
                          float *dst, void *stream);
int iamx_chain_triangulate(const int64_t *ptr, const int32_t *img, const double *uv,
                           const int32_t *group, int64_t n_chains, int group_index, const double *M,
                           const double *pos, const uint8_t *in_group, int n_images, const double *K4,
                           const double *dist5, double *ned, int32_t *status, void *stream);
int iamx_chain_pair_angles(const int64_t *ptr, const int32_t *img, const int32_t *group,
                           const double *ned, int64_t n_chains, int group_index, const double *pos,
                           const uint8_t *in_group, int n_images, double min_angle_deg, int32_t *count,
                           int64_t *total, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------
 * Surface-consistency and depth culls of chains (csrc/chain_surface.hip) -- the rules of the
 * reference's scripts/4c-surface-outliers3.py and scripts/4c-by-depth.py.  All arithmetic is f64,
 * every product and sum rounded on its own, sums left to right in the stated order; no
 * floating-point atomics, so no result depends on the launch geometry or differs between runs.
 * Pinned to tests/surface_cull_restatement.py.  All pointers DEV.  Null, size and range checks
 * return IAMX_EINVAL without a GPU; n == 0 returns 0 without a launch.
 *
 * The observation table (built by match_culling.observation_table): the members of the looked-at
 * chains whose image is in the group, image-major (a stable sort of the flattened member order by
 * image index): img_ptr [n_images + 1] i64, uv [n_obs][2] f64 (stored, distorted pixels), ned
 * [n_obs][3] f64 (the chain's position), chain [n_obs] i32.
 *
 * iamx_surface_knn_fit: per image with n observations (1 <= k, n_pos <= IAMX_SURFACE_MAX_K):
 *   n < 3: used = 0, status _SKIPPED_SMALL for each of its observations.  Otherwise per query i:
 *   d2[j] = du*du + dv*dv over the image's observations; the first min(k, n) in ascending (d2, j);
 *   walked in that order with positives = 0: a neighbour with d2 > 0 first adds 1 to positives, and
 *   positives > n_pos ends the walk in front of it; every other neighbour is used (the query itself
 *   and every duplicate pixel included).  For the m used neighbours in walk order x = sqrt(d2),
 *   y = sqrt((dx*dx + dy*dy) + dz*dz) of the two positions; xm = sum x / m, ym = sum y / m,
 *   sxx = sum (x - xm)^2, sxy = sum (x - xm)(y - ym).  sxx == 0 (or NaN): status _SKIPPED_FLAT,
 *   used = 0.  Otherwise a = sxy / sxx, b = ym - a*xm, fit = {a, b}, status _FITTED, used = m and
 *   slot s gets tgt = chain[j], val = |(a*x + b) - y|.  Slots from `used` on get tgt = -1,
 *   val = 0; a skipped query's fit is {0, 0}.  tgt [n_obs][k] i32, val [n_obs][k] f64, used
 *   [n_obs] i32, fit [n_obs][2] f64, status [n_obs] i32.  n_obs * k must fit 31 bits.
 *
 * iamx_surface_chain_metric: per chain c < n_chains: sum[c] = the val of the slots with tgt == c
 *   added in ascending (observation, slot) order, count[c] their number, metric[c] = sum / count
 *   (0 when count is 0); a tgt outside [0, n_chains) addresses nobody.  counters [4] i64:
 *   _N_SMALL / _N_FLAT (observations of that status), _N_UNCOUNTED (chains with looked[c] and
 *   count 0), _N_LOOKED.  n_chains == 0: no launch; n_obs == 0: zeros are written.  work_off
 *   [n_chains + 1] i64, work_order [n_obs * k] i32.
 *
 * iamx_chain_outlier_stats: over the chains with looked[c], n of them: average = sum metric / n,
 *   stddev = sqrt(sum (average - metric)^2 / n), both sums by a fixed tree (tiles of
 *   IAMX_CHAIN_STATS_TILE chains folded pairwise, the tiles folded by one workgroup); flag[c] =
 *   |average - metric| >= factor*stddev with two_sided, metric > average + factor*stddev without;
 *   stddev == 0 and n == 0 (average = stddev = 0) flag nothing.  stats [4] f64 (_AVERAGE, _STDDEV,
 *   _N, _BAND = factor*stddev), flag [n_chains] u8, out_idx / out_metric [n_chains]: the flagged
 *   chains in ascending order with their metric, n_flagged [1] i64.  work_part f64, work_cnt i32
 *   [ceil(n_chains / tile)], work_off i64 [that + 1].
 *
 * iamx_chain_depths: depth[o] = sqrt((dx*dx + dy*dy) + dz*dz) of ned[o] - pos[image of o]; z
 *   [n_images][3] = mean, population deviation and count of the image's depths (fixed tree; an
 *   image without observations: zeros); chain_ptr [n_chains + 1] i64 / chain_obs [n_obs] i32: the
 *   observations of each chain in member order; a chain with >= 2 of them: looked = 1, metric =
 *   the mean over them, left to right, of |depth - z mean of the image|; any other: looked = 0,
 *   metric = 0.
 * ------------------------------------------------------------------------------------ */
#define IAMX_SURFACE_MAX_K 32
#define IAMX_SURFACE_FITTED 1
#define IAMX_SURFACE_SKIPPED_SMALL 2
#define IAMX_SURFACE_SKIPPED_FLAT 3
#define IAMX_SURFACE_N_SMALL 0
#define IAMX_SURFACE_N_FLAT 1
#define IAMX_SURFACE_N_UNCOUNTED 2
#define IAMX_SURFACE_N_LOOKED 3
#define IAMX_SURFACE_N_COUNTERS 4
#define IAMX_CHAIN_STATS_TILE 256
#define IAMX_STATS_AVERAGE 0
#define IAMX_STATS_STDDEV 1
#define IAMX_STATS_N 2
#define IAMX_STATS_BAND 3
int iamx_surface_knn_fit(const int64_t *img_ptr, const double *uv, const double *ned,
                         const int32_t *chain, int n_images, int64_t n_obs, int k, int n_pos,
                         int32_t *tgt, double *val, int32_t *used, double *fit, int32_t *status,
                         void *stream);
int iamx_surface_chain_metric(const int32_t *tgt, const double *val, const int32_t *status,
                              int64_t n_obs, int k, const uint8_t *looked, int64_t n_chains,
                              double *sum, int32_t *count, double *metric, int64_t *counters,
                              int64_t *work_off, int32_t *work_order, void *stream);
int iamx_chain_outlier_stats(const double *metric, const uint8_t *looked, int64_t n_chains,
                             double factor, int two_sided, double *stats, uint8_t *flag,
                             int32_t *out_idx, double *out_metric, int64_t *n_flagged,
                             double *work_part, int32_t *work_cnt, int64_t *work_off, void *stream);
int iamx_chain_depths(const int64_t *img_ptr, const double *ned, int n_images, int64_t n_obs,
                      const double *pos, const int64_t *chain_ptr, const int32_t *chain_obs,
                      int64_t n_chains, double *depth, double *z, double *metric, uint8_t *looked,
                      void *stream);

/* ------------------------------------------------------------------------------------
 * Orthomosaic raster (csrc/ortho_raster.hip): the textured surface grids of Step 5 composed
 * top-down into one raster of H x W pixels, row 0 north.  The rules (polygons, exact coverage,
 * texture coordinate, sample, the two composition modes) are stated once in
 * imageanalysis_amd/ortho.py and restated by tests/ortho_restatement.py.  All pointers DEV unless
 * noted; null, size and range checks need no GPU.
 *
 * mode IAMX_ORTHO_BEST:    acc [H*W] f64 (the winner's metric), index [H*W] i32 (-1: uncovered),
 *                          count [H*W] u16, bgr [H*W][3] u8 written by the raster kernel itself.
 * mode IAMX_ORTHO_FEATHER: acc [H*W][4] f64 (sum w b, sum w g, sum w r, sum w; 32-byte aligned),
 *                          index unused (may be NULL), count as above, bgr written by resolve.
 *
 * clear:        the accumulators' start values (best: metric +inf, index -1; feather: zeros).
 * raster_image: one image per launch, stream ordered -- the images of a group are composed in the
 *   order of the calls.  X, Y i32 [(S+1)^2]: vertices snapped to 1/256 pixel; uv f64 [(S+1)^2][2]:
 *   source pixels in the camera's size; used u8 [S^2]: the cells that count; frame u8
 *   [h_s][w_s][3]; params HOST f64 [8] = camera width, height, raster x0, y1, gsd, the image's
 *   centre east, north and 0.1 span (the last three read in mode best only); image_index: what
 *   `index` receives; c0, r0, c1, r1: the inclusive pixel box of the image's used vertices
 *   (c1 < c0 or r1 < r0: nothing is launched).  1 <= S <= iamx_ortho_max_steps().
 * resolve:      feather only: bgr = floor(sum w colour / sum w + 0.5) where count > 0.
 * ------------------------------------------------------------------------------------ */
#define IAMX_ORTHO_BEST 0
#define IAMX_ORTHO_FEATHER 1
int iamx_ortho_max_steps(void);
int iamx_ortho_clear(int mode, int H, int W, double *acc, int32_t *index, uint16_t *count,
                     uint8_t *bgr, void *stream);
int iamx_ortho_raster_image(int mode, int S, const int32_t *X, const int32_t *Y, const double *uv,
                            const uint8_t *used, const uint8_t *frame, int h_s, int w_s,
                            const double *params, int image_index, int c0, int r0, int c1, int r1,
                            int H, int W, double *acc, int32_t *index, uint16_t *count, uint8_t *bgr,
                            void *stream);
int iamx_ortho_resolve(int H, int W, const double *acc, const uint16_t *count, uint8_t *bgr,
                       void *stream);

/* Mode multiband (Laplacian pyramids, float32; the rules: imageanalysis_amd/ortho.py, restated by
 * tests/ortho_multiband_restatement.py).  It has entry points of its own: the mode numbers of the
 * calls above stay 0 and 1.  Level l of an H x W mosaic is h x w with h_0 = H, h_{l+1} =
 * (h_l + 1) / 2.  A pixel of a level is four floats, 16-byte aligned: a LAYER holds (C_b, C_g, C_r,
 * A) of one image and lives in a buffer of its REGION only, an inclusive box (y0, x0, y1, x1) of
 * the level, row-major; outside its region a layer is 0.  An ACCUMULATOR holds (N_b, N_g, N_r, D)
 * over the whole level.  All pointers DEV unless noted; every check is made on the host first.
 *
 * owner:       mode best's count, metric and index from the geometry alone (no frame, no bgr): what
 *   iamx_ortho_raster_image(0, ...) leaves in acc, index and count, after iamx_ortho_clear(0, ...).
 * layer:       level 0 of image `image_index` over its pixel box (c0, r0, c1, r1), which is the
 *   layer's region: C = the sample (float64 cast to float32) where the image covers the pixel,
 *   A = 1 where index == image_index, 0 elsewhere.  Arguments as iamx_ortho_raster_image's.
 * reduce:      dst = R(src) over the region (dy0 .. dx1) of the level below the h x w one, src given
 *   over (sy0 .. sx1): taps (1, 4, 6, 4, 1) / 16 at 2j - 2 .. 2j + 2, along x first, then along y.
 * accumulate:  over the region (fy0 .. fx1) of the h x w level: LP = C(fine) - E(C(coarse)), or
 *   LP = C(fine) when coarse is null (the top level); N += A LP, D += A into acc [h][w][4].
 * collapse:    one level, whole: M = N / D (0 where D == 0) + E(M of the level below, `up`
 *   [(h+1)/2][(w+1)/2][4], null at the top level).  bgr null: M replaces N in acc.  bgr given
 *   (level 0): bgr = floor(min(max(M, 0), 255) + 0.5) where count > 0, else 0; acc is left alone.
 */
int iamx_ortho_mb_owner(int S, const int32_t *X, const int32_t *Y, const uint8_t *used,
                        const double *params, int image_index, int c0, int r0, int c1, int r1, int H,
                        int W, double *metric, int32_t *index, uint16_t *count, void *stream);
int iamx_ortho_mb_layer(int S, const int32_t *X, const int32_t *Y, const double *uv,
                        const uint8_t *used, const uint8_t *frame, int h_s, int w_s,
                        const double *params, int image_index, int c0, int r0, int c1, int r1, int H,
                        int W, const int32_t *index, float *layer, void *stream);
int iamx_ortho_mb_reduce(int h, int w, const float *src, int sy0, int sx0, int sy1, int sx1,
                         float *dst, int dy0, int dx0, int dy1, int dx1, void *stream);
int iamx_ortho_mb_accumulate(int h, int w, const float *fine, int fy0, int fx0, int fy1, int fx1,
                             const float *coarse, int cy0, int cx0, int cy1, int cx1, float *acc,
                             void *stream);
int iamx_ortho_mb_collapse(int h, int w, float *acc, const float *up, const uint16_t *count,
                           uint8_t *bgr, void *stream);

/* ------------------------------------------------------------------------------------
 * RANSAC verification of pair matches -- scripts/lib/matcher.py:90-142 filter_by_transform()
 * (cv2.findHomography / cv2.findFundamentalMat with cv2.RANSAC).  Parity with cv2 is UNPINNED:
 * cv2's sample sequence is its own; this one is the stateless rule of csrc/verify_rule.h.
 *
 * One workgroup per pair.  Pair p owns matches m_off[p] .. m_off[p+1]-1 of pts; a pair's result
 * depends on its own points, tol[p], model, hypotheses and seed only, never on its place in the
 * batch.  Everything is f64 on the float32 points widened:
 *   1. Hartley normalisation per image (centroid, mean distance sqrt 2), fixed reduction trees;
 *      all points of an image coincident (or not finite) -> IAMX_VERIFY_NO_MODEL.
 *   2. hypothesis h < hypotheses: k matches by verify_sample (k = 4 homography, 8 fundamental), the
 *      8x9 system in normalised coordinates
 *        homography, two rows per match: [-x -y -1 0 0 0 ux uy u], [0 0 0 -x -y -1 vx vy v]
 *        fundamental, one row per match: [ux uy u vx vy v x y 1]
 *      and its null vector by Gauss-Jordan over the nine columns in order: column c takes the unused
 *      row of largest |a| (ties: the lowest row) as its pivot; a pivot of at most 2^-40 times the
 *      largest |entry| of the system leaves the column FREE; otherwise every other row, used ones
 *      included, is reduced in all columns.  Then the last free column is 1, the other free columns
 *      0, and each pivot column follows from its row.  A rank-deficient sample still gives a member
 *      of its null space.
 *   3. fundamental: the smallest singular value zeroed (one-sided Jacobi, eight sweeps), then
 *      M = T2^T M T1.  Homography: M = T2^-1 M T1.  M is scaled to unit Frobenius norm with its
 *      largest-magnitude entry positive; a model with an entry that is not finite is passed over.
 *   4. error of every match: homography |pi(M x1) - x2|^2 (w zero or not finite: outlier);
 *      fundamental max(e^2 / (l1x^2 + l1y^2), e^2 / (l2x^2 + l2y^2)), e = x2^T M x1, l2 = M x1,
 *      l1 = M^T x2.  Inlier: err <= tol^2; a NaN never is.
 *   5. the hypothesis with the most inliers, ties to the lowest h.  No refit, no adaptive stop.
 * pts must be 16-byte aligned.  A pair whose offsets leave [0, total], or with 2^31 matches or
 * more, gets status NO_MODEL and nothing of it is read or written.  n_pairs == 0 returns IAMX_OK
 * without a launch.
 *
 * iamx_verify_sample (host): the k indices hypothesis hyp draws out of n, in draw order.
 * 1 <= k <= 8, k <= n < 2^31, hyp >= 0.
 * ------------------------------------------------------------------------------------ */
#define IAMX_VERIFY_HOMOGRAPHY 0
#define IAMX_VERIFY_FUNDAMENTAL 1
#define IAMX_VERIFY_OK 0        /* a model was chosen, mask written                       */
#define IAMX_VERIFY_TOO_FEW 1   /* n < sample size: mask all 1, model NaN, best -1        */
#define IAMX_VERIFY_NO_MODEL 2  /* no hypothesis with a finite model and >= 1 inlier: mask all 0,
                                   model NaN, best (-1, 0)                                 */
int iamx_verify_pairs(const float *pts,      /* DEV [total][4] x1 y1 x2 y2 (undistorted px) */
                      const int64_t *m_off,  /* DEV [n_pairs+1] */
                      int n_pairs, int64_t total, int model,
                      const double *tol,     /* DEV [n_pairs] px */
                      int hypotheses, uint64_t seed,
                      uint8_t *mask,         /* DEV [total] */
                      double *out_model,     /* DEV [n_pairs][9] row major, unit Frobenius norm,
                                                largest-magnitude entry positive */
                      int32_t *out_best,     /* DEV [n_pairs][2] hypothesis index, inlier count */
                      int32_t *status,       /* DEV [n_pairs] */
                      void *stream);
int iamx_verify_sample(int64_t n, int k, int64_t hyp, uint64_t seed, int32_t *out /* HOST [k] */);

/* ------------------------------------------------------------------------------------
 * The essential model -- cv2.findEssentialMat in the same filter -- as an entry of its own.
 * iamx_verify_pairs keeps refusing model 2.  Departures from cv2, parity UNPINNED: the error is the
 * symmetric epipolar distance in pixels under F = K^-T E K^-1 (cv2: Sampson on rays), the number
 * of hypotheses is fixed, the sample sequence is verify_sample's.
 *
 * K is a HOST array [9], row major: [fx skew cu; 0 fy cv; 0 0 1].  K[3], K[6], K[7] must be 0,
 * K[8] must be 1, fx and fy finite and not zero; a skew is allowed.  These and the pointer,
 * alignment and size checks of iamx_verify_pairs are made before any launch; n_pairs == 0 returns
 * IAMX_OK without one.
 *
 * One workgroup per pair, everything f64 on the float32 points widened:
 *   1. rays: y = (v - cv) / fy, x = ((u - cu) - skew y) / fx.  No Hartley normalisation.
 *   2. hypothesis h < hypotheses draws k = 5 matches by verify_sample.
 *   3. the 5x9 system, one row per match [ux uy u vx vy v x y 1] ((x, y) image 1, (u, v) image 2),
 *      and its null space by Gauss-Jordan with FULL pivoting: five times the largest |a| over the
 *      unused rows and columns (ties: the lowest row, then the lowest column); a pivot of at most
 *      2^-40 times the largest |entry| of the system means rank < 5 and the hypothesis is passed
 *      over; otherwise every other row is reduced in all columns.  The four free columns in
 *      ascending order give the basis X, Y, Z, W: its own free column 1, the other free columns 0,
 *      each pivot column -a[row][free] / a[row][pivot].
 *   4. E = xX + yY + zZ + W.  Ten cubic constraints, row 0 det E (first row expansion), rows
 *      1 + 3i + j the entries of (E E^T - tr(E E^T)/2) E, as a 10x20 matrix over the monomials
 *        leading   x3 x2y xy2 y3 x2z x2 xyz xy y2z y2
 *        trailing  xz2 xz x yz2 yz y z3 z2 z 1
 *      Gauss-Jordan of the leading 10x10 block column by column: the row of largest |a| among rows
 *      c .. 9 (ties: the lowest) is swapped into place c, divided by its pivot, and taken out of
 *      every other row.  A pivot of at most 2^-40 times the largest |entry| of the matrix: passed
 *      over.
 *   5. row(x2z) - z row(x2), row(xyz) - z row(xy), row(y2z) - z row(y2) are B(z) [x y 1]^T = 0
 *      with entries of degree 3, 3, 4; p(z) = det B(z) (first row expansion) has degree 10.
 *   6. real roots of p, no randomness, the same operations for the same input: R = 1 + max |c_i| /
 *      |c_10| (Cauchy).  A coefficient or R that is not finite, or c_10 = 0: passed over.  For
 *      k = 1 .. 10 the derivative q = p^(10-k) has degree k; the roots found for p^(11-k), with -R
 *      in front and R behind, cut [-R, R] into intervals.  An interval [a, b] holds a root of q
 *      where (q(a) < 0) != (q(b) < 0) (Horner); it is bisected 32 times (48 for p itself, k = 10),
 *      mid = (lo + hi) / 2 replacing the end whose sign it shares, and the root is the last
 *      interval's middle.  For p itself two Newton steps z - p(z) / p'(z) follow, each kept only
 *      where it stays inside [a, b].  Roots come out in ascending z, at most ten.
 *   7. per root: B(z) numerically; of the cross products of its rows (0,1), (0,2), (1,2) the
 *      first of largest norm is proportional to [x y 1]; E follows and is scaled to unit Frobenius
 *      norm with its largest-magnitude entry positive.  F = K^-T E K^-1 in closed form (a = 1/fx,
 *      d = 1/fy, b = -(skew d) a, c = -(a cu + b cv), e = -(d cv); G = E K^-1, F = K^-T G), scaled
 *      the same way.  A candidate whose E or F has an entry that is not finite is passed over.
 *   8. every candidate is scored with the fundamental model's error on the pixel F, tol in
 *      pixels; the most inliers win, ties to the lowest hypothesis, then the earliest root.  No
 *      cheirality test, no refit, no adaptive stop.
 * n < 5: IAMX_VERIFY_TOO_FEW.  No candidate with an inlier (every sample of identical matches is
 * rank deficient): IAMX_VERIFY_NO_MODEL.  Both write mask, model and best as iamx_verify_pairs
 * does; out_essential, where given, is NaN wherever out_model is.
 *
 * iamx_five_point: steps 3 to 7 alone, one sample per lane, the same device function.  E[s][r] is
 * the r-th model of sample s on its rays (unit norm, largest entry positive, ascending z);
 * entries past count[s] are NaN.  count is 0 for a sample that is passed over.
 * ------------------------------------------------------------------------------------ */
#define IAMX_VERIFY_ESSENTIAL 2
int iamx_verify_pairs_essential(const float *pts,      /* DEV [total][4] x1 y1 x2 y2 (undistorted px) */
                                const int64_t *m_off,  /* DEV [n_pairs+1] */
                                int n_pairs, int64_t total,
                                const double *K,       /* HOST [9] row major */
                                const double *tol,     /* DEV [n_pairs] px */
                                int hypotheses, uint64_t seed,
                                uint8_t *mask,         /* DEV [total] */
                                double *out_model,     /* DEV [n_pairs][9]: F = K^-T E K^-1 in pixels */
                                double *out_essential, /* DEV [n_pairs][9] or NULL: E on normalised rays */
                                int32_t *out_best,     /* DEV [n_pairs][2] hypothesis index, inlier count */
                                int32_t *status,       /* DEV [n_pairs] */
                                void *stream);
int iamx_five_point(const double *rays, /* DEV [n][5][4] x1 y1 x2 y2, normalised */
                    int n,
                    double *E,          /* DEV [n][10][9] */
                    int32_t *count,     /* DEV [n] */
                    void *stream);

/* ------------------------------------------------------------------------------------
 * The 'bestratio' strategy -- scripts/lib/matcher.py:595-694 ratio_pair_matches(): ONE direction
 * of every pair, Lowe-ratio bins, a RANSAC homography per bin, the bin with the most unique inliers.
 * Three launches: iamx_ratio_bins, iamx_verify_pairs(model = homography) over the n_pairs * n_bins
 * segments it leaves, iamx_ratio_select.  The Python-level rules are the reference's; the consensus
 * is iamx_verify_pairs' rule (parity with cv2 UNPINNED).
 *
 * iamx_ratio_bins, one workgroup per ordered pair over its top-2 rows (iamx_knn2_l2_pairs):
 *   idx / d2  DEV [total rows][2]; row_off DEV [n_pairs + 1] int64 first row of every pair;
 *   pairs DEV [n_pairs][2] image slots (query, train); kp_off / xy as for iamx_match_postfilter;
 *   cutoffs HOST [n_bins] doubles, ascending, 1 <= n_bins <= 8.
 *   ratio = (double)d0 / (double)d1 with d* = float32(sqrt(d2*)); bin b holds the rows with
 *   ratio <= cutoffs[b] in query-row order; a row with d1 == 0 is in no bin and adds 1 to flag[0]
 *   (python divides by it: the caller raises ZeroDivisionError).
 *   bin_cnt DEV [n_pairs][n_bins] members of every bin.  seg_cnt DEV [n_pairs][n_bins]: the same
 *   where the bin is looked at -- at least min_pairs members (matcher.py:634) and at least 4 (a
 *   homography's sample), and not as many as the last bin that was looked at (nested bins: the
 *   same set, the same consensus, which cannot win under `>`) -- else 0.  seg_off DEV
 *   [n_pairs * n_bins + 1] int64: exclusive scan of seg_cnt = the m_off of iamx_verify_pairs.
 *   pts DEV [cap][4] x1 y1 x2 y2 = kp.pt of both ends (16-byte aligned), rows DEV [cap][2]
 *   (query row, train row); cap >= n_bins * total rows.  flag DEV [2] is only ever raised:
 *   [0] rows with d1 == 0, [1] pairs refused (more than 2^24 rows, or a size the caller got wrong).
 *
 * iamx_ratio_select, one workgroup per pair, over mask / status of iamx_verify_pairs:
 *   per bin in order: the inliers in order (none where status != IAMX_VERIFY_OK), their number
 *   `fit`, and `unique` = what filter_duplicates (matcher.py:157-182: first come wins on key2 of
 *   either end, a dropped entry reserves no key) leaves of them; the bin is taken where unique is
 *   strictly more than the best so far (min_unique = 20 at the start).  The result is the taken
 *   bin's de-duplicated list if its fit and its unique are both >= min_pairs, else empty.
 *   stats DEV [n_pairs][n_bins][3] = members, fit, unique (-1, -1 where the bin is not looked at; a
 *   bin that repeats the one before carries that one's figures); chosen DEV [n_pairs] (-1: none);
 *   out_slots DEV [n_pairs][stride][2] and out_cnt DEV [n_pairs]: the lists in fixed slots (what
 *   iamx_similarity_pairs reads with clip = stride); out_off DEV [n_pairs + 1] int64 and out_rows
 *   DEV [out_cap][2]: the same lists packed back to back (out_cap >= total rows).
 *   There is no clip here: stride >= the rows of the largest query image of the launch, tab_size a
 *   power of two >= max(64, 2 * stride), work DEV [n_pairs][6 * stride + 2 * tab_size] int32.
 * Null pointers, negative counts and n_bins outside 1..8: IAMX_EINVAL without a launch.
 * ------------------------------------------------------------------------------------ */
int iamx_ratio_bins(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                    const int32_t *pairs, const int64_t *kp_off, const float *xy, int n_pairs,
                    int n_bins, const double *cutoffs, double min_pairs, int64_t cap,
                    int32_t *bin_cnt, int32_t *seg_cnt, int64_t *seg_off, float *pts, int32_t *rows,
                    int32_t *flag, void *stream);
int iamx_ratio_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2, int n_pairs,
                      int n_bins, double min_pairs, int min_unique, const int32_t *bin_cnt,
                      const int32_t *seg_cnt, const int64_t *seg_off, const int32_t *rows,
                      const uint8_t *mask, const int32_t *vstatus, int64_t cap, int stride,
                      int tab_size, int32_t *work, int32_t *out_slots, int32_t *out_cnt,
                      int64_t *out_off, int32_t *out_rows, int64_t out_cap, int32_t *chosen,
                      int32_t *stats, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------
 * The 'smart' strategy -- scripts/lib/matcher.py:358-593 smart_pair_matches(): a homography
 * predicted from the camera poses picks, among every feature's three nearest neighbours
 * (iamx_knn3_l2_pairs), the one nearest to the prediction; a RANSAC homography per distance bin
 * tightens the prediction until no bin gains unique inliers.  One pass of the loop (:474-580) is
 * iamx_smart_stats, iamx_verify_pairs(model = homography) over the n_pairs * IAMX_SMART_BINS
 * segments it leaves, iamx_smart_select.  The Python-level rules are the reference's; the consensus is
 * iamx_verify_pairs' rule and the refit is iamx_homography_fit's (parity with cv2 UNPINNED).
 *
 * iamx_homography_fit, one workgroup per segment: the least-squares homography x2 ~ H x1 of the
 * segment's points -- cv2's kernel (HomographyEstimatorCallback::runKernel) without its LM polish:
 *   both sides normalised (centroid, mean distance sqrt 2), the 9 x 9 L^T L of the rows
 *   [X Y 1 0 0 0 -xX -xY -x], [0 0 0 X Y 1 -yX -yY -y] summed in f64 (fixed reduction trees), the
 *   eigenvector of its least eigenvalue by 12 sweeps of cyclic Jacobi, H = T2^-1 H0 T1 divided by h22.
 *   pts DEV [total][4] x1 y1 x2 y2 (16-byte aligned); seg_off DEV [n_seg + 1] int64; mask DEV [total]
 *   or NULL: only points with a non-zero mask byte count.  H DEV [n_seg][9] row major, status DEV
 *   [n_seg]: IAMX_FIT_TOO_FEW below 4 points, IAMX_FIT_DEGENERATE where a side's points coincide,
 *   an entry of the result is not finite (a NaN among the points, h22 == 0) or the segment's
 *   offsets leave [0, total]; H is NaN wherever status != IAMX_FIT_OK.
 *
 * iamx_smart_stats, one workgroup per ordered pair over its top-3 rows:
 *   idx / d2 DEV [total rows][3]; row_off, pairs, kp_off, xy, cap, pts, rows, flag as for
 *   iamx_ratio_bins; size DEV [total kp] float32 kp.size beside xy; H DEV [n_pairs][9] f64 the pair's
 *   current prediction; active DEV [n_pairs] int32 or NULL (all): a pair with active == 0 gets
 *   bin_cnt = seg_cnt = 0 and nothing else.
 *   Query row i: p1 = pi(H kp.pt) in doubles with the quotient taken by the reciprocal, stored as
 *   float32, (0, 0) where w == 0 (cv2.perspectiveTransform).  Neighbours j = 0, 1, 2 in order, with
 *   d* = float32(sqrt(d2*)): stop at d2[j] >= 90000 (distance >= 300; a missing neighbour); ratio =
 *   (double)d0 / (double)dj, stop at ratio < match_ratio; raw_dist = float32 |kp2.pt - p1| (float32
 *   differences, squares and sum, then the correctly rounded root); size_diff = the larger of the two
 *   kp.size over the smaller as doubles, the neighbour is passed over at size_diff > 1.25; metric =
 *   (double)raw_dist * size_diff / ratio; the first neighbour that gets here is the row's choice, a
 *   later one replaces it at a strictly smaller metric.  The choice is in bin b where its raw_dist <
 *   32 << b, in query-row order.  A row with d2[0] == 0 has no choice and adds 1 to flag[0] (python
 *   divides 0.0 by 0.0: the caller raises ZeroDivisionError).
 *   bin_cnt / seg_cnt / seg_off as for iamx_ratio_bins with n_bins = IAMX_SMART_BINS.
 *
 * iamx_smart_select, one workgroup per pair, over mask / status / model of iamx_verify_pairs:
 *   the walk of iamx_ratio_select with the pair's running best READ from and written to best DEV
 *   [n_pairs][2] = (unique, fitted) of the pair's list (the caller starts it at (20, 0)).  A bin with
 *   strictly more unique inliers than the best so far becomes the pair's list -- out_slots holds its
 *   de-duplicated inliers, out_cnt their number where fitted and unique are both >= min_pairs (else
 *   0) -- and improved DEV [n_pairs] is 1 + the last such bin of the walk.  A pair without such a
 *   bin keeps best, out_slots, out_cnt and H as they are and gets improved = 0; so does a pair with
 *   active == 0, whose stats stay too.  For a pair that improved, the taken bin's inliers go through
 *   iamx_homography_fit's kernel: H DEV [n_pairs][9] becomes the fit, or vmodel's model of the bin
 *   where fit_status DEV [n_pairs] is not IAMX_FIT_OK.  stats, out_off, out_rows, stride, tab_size,
 *   work as for iamx_ratio_select; out_off / out_rows are packed on every call from out_cnt /
 *   out_slots.  The loop ends when no pair improves: best strictly rises and cannot pass the rows.
 * Null pointers, negative counts, a stride or tab_size out of range: IAMX_EINVAL without a launch.
 * ------------------------------------------------------------------------------------ */
#define IAMX_SMART_BINS 7
#define IAMX_FIT_OK 0
#define IAMX_FIT_TOO_FEW 1
#define IAMX_FIT_DEGENERATE 2
int iamx_homography_fit(const float *pts, const int64_t *seg_off, const uint8_t *mask, int n_seg,
                        int64_t total, double *H, int32_t *status, void *stream);
int iamx_smart_stats(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                     const int32_t *pairs, const int64_t *kp_off, const float *xy, const float *size,
                     const double *H, const int32_t *active, int n_pairs, double match_ratio,
                     double min_pairs, int64_t cap, int32_t *bin_cnt, int32_t *seg_cnt,
                     int64_t *seg_off, float *pts, int32_t *rows, int32_t *flag, void *stream);
int iamx_smart_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2,
                      const int32_t *active, int n_pairs, double min_pairs, const int32_t *bin_cnt,
                      const int32_t *seg_cnt, const int64_t *seg_off, const float *pts,
                      const int32_t *rows, const uint8_t *mask, const int32_t *vstatus,
                      const double *vmodel, int64_t cap, int stride, int tab_size, int32_t *work,
                      int32_t *best, int32_t *improved, int32_t *out_slots, int32_t *out_cnt,
                      int64_t *out_off, int32_t *out_rows, int64_t out_cap, int32_t *stats, double *H,
                      int32_t *fit_status, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------
 * The 'bruteforce' strategy -- scripts/lib/matcher.py:696-850 bruteforce_pair_matches(): ONE
 * direction of every pair, no pose prior.  Among every feature's three nearest neighbours
 * (iamx_knn3_l2_pairs) the one of the smallest size_diff / ratio; the choices grouped by their
 * image-space motion into 41 x 21 overlapping (length, direction) cells; a RANSAC homography per
 * cell; the cell with the most fitted inliers, the distance bins walked with the reference's early
 * exit.  Three launches: iamx_brute_bins, iamx_verify_pairs(model = homography) over the n_pairs *
 * IAMX_BRUTE_CELLS segments it leaves, iamx_brute_select.  The Python-level rules are the
 * reference's; the consensus is iamx_verify_pairs' rule (parity with cv2 UNPINNED).
 *
 * iamx_brute_bins, one workgroup per ordered pair over its top-3 rows:
 *   idx / d2 DEV [total rows][3]; row_off, pairs, kp_off, xy, size, pts, rows, flag as for
 *   iamx_smart_stats.  step_d = int(diag * 0.55) / 40 with diag = int(sqrt(h * h + w * w)) and
 *   step_a = 2 pi / 20, computed by the caller as doubles; both positive and finite.
 *   Query row i: neighbours j = 0, 1, 2 in order, with d* = float32(sqrt(d2*)): stop at d2[j] >=
 *   84100 (distance >= 290; a missing neighbour, idx -1 / d2 0x7FFFFFFF, too); ratio = (double)d0 /
 *   (double)dj, stop at ratio < match_ratio; v = kp2.pt - kp1.pt in float32; raw_dist = the
 *   correctly rounded float32 root of the float32 sum of v's squares; size_diff = the larger of the
 *   two kp.size over the smaller as doubles, the neighbour is passed over (not a stop) at size_diff >
 *   1.25; metric = size_diff / ratio; the first neighbour that gets here is the row's choice, a later
 *   one replaces it at a strictly smaller metric.  vangle = atan2((double)v.y, (double)v.x), plus
 *   2 pi where it is negative (-0.0 is not).  A row with d2[0] == 0 has no choice and adds 1 to
 *   flag[0] (python divides 0.0 by 0.0: the caller raises ZeroDivisionError).
 *   dbin = rint((double)raw_dist / step_d), round-half-even -- a FLOAT64 quotient: the reference's
 *   environment pins NumPy 1.20, where np.float32 / float is one (under NumPy 2 the same expression
 *   is a float32 quotient; the goldens refuse every row on which the two differ).  A row with dbin >
 *   40 is in no cell; else it is in distance bins dbin, dbin - 1 (dbin > 0) and dbin + 1 (dbin < 40).
 *   abin = rint(vangle / step_a) in 0..20; the row is in angle bins abin - 1, abin, abin + 1, for
 *   abin == 0 in 20, 0, 1 and for abin == 20 in 19, 20, 0 (matcher.py:785-795 as it stands).  So a
 *   row is in up to nine of the cells dbin * 21 + abin, once in each, and every cell's members are
 *   in QUERY-ROW ORDER (the consensus' sample sequence and filter_duplicates depend on it).
 *   bin_cnt DEV [n_pairs][861] members of every cell.  seg_cnt DEV [n_pairs][861]: the same where
 *   the cell is looked at -- at least min_pairs members (matcher.py:797) and at least 4 (a
 *   homography's sample) -- else 0.  seg_off DEV [n_pairs * 861 + 1] int64: exclusive scan of seg_cnt
 *   = the m_off of iamx_verify_pairs.  pts DEV [cap][4] / rows DEV [cap][2]: the looked-at cells;
 *   cap >= 9 * total rows.  A pair of more than 2^24 rows gets nothing and adds 1 to flag[1].
 *
 * iamx_brute_select, one workgroup per pair, over mask / status of iamx_verify_pairs:
 *   distance bins 0..40 in order, within each the angle bins 0..20 in order.  A looked-at cell's
 *   num_fit is its inlier count (0 where status != IAMX_VERIFY_OK); best_of_bin the largest num_fit of
 *   the distance bin (0 without a looked-at cell); a cell with num_fit strictly above the best so far
 *   (0 at the start) becomes the pair's list -- the comparison is on FITTED inliers, not unique ones,
 *   unlike iamx_ratio_select.  After each distance bin the walk stops at best > 50 && best_of_bin <
 *   10.  After the walk: the taken cell's inliers in order if they are at least min_pairs, through
 *   filter_duplicates (as for iamx_ratio_select), kept if at least min_pairs remain, else empty.
 *   chosen DEV [n_pairs]: the taken cell dbin * 21 + abin, or -1.  stats DEV [n_pairs][4] = fitted
 *   (the best; 0 without a taken cell), unique (-1 where filter_duplicates did not run), distance bins
 *   walked, cells looked at within them.  fit_cnt DEV [n_pairs][861]: num_fit, -1 where the cell is
 *   not looked at or not reached.  out_slots / out_cnt / out_off / out_rows / out_cap, stride,
 *   tab_size, work as for iamx_ratio_select.
 * Null pointers, negative counts, a step, stride or tab_size out of range: IAMX_EINVAL without a
 * launch; n_pairs == 0: IAMX_OK without one, and nothing is written (out_off[0] included).
 * ------------------------------------------------------------------------------------ */
#define IAMX_BRUTE_DIST_BINS 41
#define IAMX_BRUTE_ANGLE_BINS 21
#define IAMX_BRUTE_CELLS 861
int iamx_brute_bins(const int32_t *idx, const int32_t *d2, const int64_t *row_off,
                    const int32_t *pairs, const int64_t *kp_off, const float *xy, const float *size,
                    int n_pairs, double match_ratio, double min_pairs, double step_d, double step_a,
                    int64_t cap, int32_t *bin_cnt, int32_t *seg_cnt, int64_t *seg_off, float *pts,
                    int32_t *rows, int32_t *flag, void *stream);
int iamx_brute_select(const int32_t *pairs, const int64_t *kp_off, const int32_t *key2, int n_pairs,
                      double min_pairs, const int32_t *seg_cnt, const int64_t *seg_off,
                      const int32_t *rows, const uint8_t *mask, const int32_t *vstatus, int64_t cap,
                      int stride, int tab_size, int32_t *work, int32_t *out_slots, int32_t *out_cnt,
                      int64_t *out_off, int32_t *out_rows, int64_t out_cap, int32_t *chosen,
                      int32_t *stats, int32_t *fit_cnt, int32_t *flag, void *stream);

/* ------------------------------------------------------------------------------------
 * Dense surface (csrc/dense_sweep.hip) -- plane-sweep depth maps, their cross-view check and
 * the DSM splat.  The rules are stated in imageanalysis_amd/dense.py ("THE RULES") and restated in
 * numpy by tests/dense_restatement.py; the device follows them bit for bit.  All pointers DEV.
 *
 * A camera is IAMX_DENSE_CAM_DOUBLES doubles: R[9] (NED -> camera, row-major), C[3] (centre, NED),
 * fx, fy, cx, cy at the sweep scale, k1, k2, p1, p2, k3.  rays [h][w][2] are a view's undistorted
 * normalised coordinates (xn, yn) at its pixel centres.
 *
 * iamx_dense_sweep, one launch per reference image: ref [h][w] float32 grey, nbr [num_nbr][h][w],
 *   ref_pose [12] = R, C of the reference, nbr_cam [num_nbr][21].  planes 1..IAMX_DENSE_MAX_PLANES
 *   uniform in inverse depth from w_far to w_near, radius 1..IAMX_DENSE_MAX_RADIUS, the texture
 *   gate min_var, the keep threshold min_score.  -> plane [h][w] (-1: every plane invalid), score
 *   [h][w] (the winner's; NaN), depth [h][w] (NaN where not kept), around [h][w][3] = the scores at
 *   plane - 1, plane, plane + 1 (NaN where there is none or it is invalid).  Every pixel is written.
 *   A workgroup owns IAMX_DENSE_TILE_W x IAMX_DENSE_TILE_H pixels.
 * iamx_dense_check, one thread per pixel of depth [V][h][w]: nbr [V][max_nbr] view numbers, -1 for
 *   none.  -> keep [V][h][w] 0 / 1, ned [V][h][w][3] the pixel's NED point (NaN where depth is).
 * iamx_dense_splat: ned [N][3], keep [N] or null (all); the points with keep != 0 inside the frame
 *   (x0 = west side of column 0, y1 = north side of row 0, gsd) add 1 to count [H][W] and
 *   rint(up 1024) to sum [H][W] by integer atomics; the caller zeroes both.  A point whose
 *   |rint(up 1024)| is above 1e15 or NaN is dropped.
 * iamx_dense_resolve: dsm [H][W] = float32(sum / 1024 / count), NaN where count == 0.
 * A size or a parameter out of range, a null pointer: IAMX_EINVAL without a launch.
 * ------------------------------------------------------------------------------------ */
#define IAMX_DENSE_TILE_W 32
#define IAMX_DENSE_TILE_H 16
#define IAMX_DENSE_MAX_RADIUS 7
#define IAMX_DENSE_MAX_PLANES 4096
#define IAMX_DENSE_MAX_NEIGHBOURS 16
#define IAMX_DENSE_MAX_SIDE 16384
#define IAMX_DENSE_MAX_RASTER 1048576
#define IAMX_DENSE_CAM_DOUBLES 21
int iamx_dense_sweep(const float *ref, const double *rays, const float *nbr, const double *ref_pose,
                     const double *nbr_cam, int width, int height, int num_nbr, int planes,
                     double w_far, double w_near, int radius, float min_var, float min_score,
                     int32_t *plane, float *score, float *depth, float *around, void *stream);
int iamx_dense_check(const float *depth, const double *rays, const double *cams, const int32_t *nbr,
                     int num_views, int max_nbr, int width, int height, double eps, int min_agree,
                     uint8_t *keep, double *ned, void *stream);
int iamx_dense_splat(const double *ned, const uint8_t *keep, int64_t num_points, double x0, double y1,
                     double gsd, int width, int height, int32_t *count, int64_t *sum, void *stream);
int iamx_dense_resolve(const int32_t *count, const int64_t *sum, int width, int height, float *dsm,
                       void *stream);

/* ------------------------------------------------------------------------------------
 * Dense surface, semi-global aggregation (csrc/dense_sgm.hip, the emission in csrc/dense_sweep.hip):
 * the layer between the sweep's cost volume and the winner.  The rules are stated in
 * imageanalysis_amd/dense.py ("SEMI-GLOBAL RULES") and restated in numpy by
 * tests/dense_sgm_restatement.py; the device follows them bit for bit.  All pointers DEV.
 *
 * volume [h][w][planes] uint8, planes contiguous: the cost C of (pixel, plane), 255 where the sweep's
 * aggregate score is invalid, else clamp(rint((1 - S) 127), 0, 254).  total [h][w][planes] uint16:
 * the sum T of the directions' path costs, at most 8 (254 + 255) = 4072.  2 <= planes <=
 * IAMX_DENSE_SGM_MAX_PLANES (one plane per lane of a wave).
 *
 * iamx_dense_sweep_volume: iamx_dense_sweep with the same arguments and the same four outputs, and
 *   volume written beside them (every pixel, every plane); volume is aligned to 4 bytes.
 * iamx_dense_sgm_direction, one launch: the path costs L_r of direction 0 .. 7 (in the rules' order:
 *   (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1) (-1,1) as (dx, dy)), one wave per path; accumulate
 *   0: total = L_r (every element is written), else total += L_r.  0 <= p1 <= p2 <= 255, c_invalid
 *   0 .. 254 stands in for a cost of 255.
 * iamx_dense_sgm_paths: the first `paths` (4 or 8) directions, stream ordered, the first one storing
 *   and the others adding: total needs no zeroing by the caller and nothing of its old content stays.
 * iamx_dense_sgm_select, one wave per pixel: plane [h][w] = argmin_d T (the smallest d on a tie, never
 *   -1), cost [h][w] = the raw C there, tot0 [h][w] = T there, depth [h][w] = the sub-plane depth
 *   where cost <= max_cost (0 .. 254), NaN elsewhere; step = (w_near - w_far) / (planes - 1) > 0.
 * A size or a parameter out of range, a null pointer: IAMX_EINVAL without a launch.
 * ------------------------------------------------------------------------------------ */
#define IAMX_DENSE_SGM_MAX_PLANES 64
int iamx_dense_sweep_volume(const float *ref, const double *rays, const float *nbr,
                            const double *ref_pose, const double *nbr_cam, int width, int height,
                            int num_nbr, int planes, double w_far, double w_near, int radius,
                            float min_var, float min_score, int32_t *plane, float *score, float *depth,
                            float *around, uint8_t *volume, void *stream);
int iamx_dense_sgm_direction(const uint8_t *volume, int width, int height, int planes, int direction,
                             int accumulate, int p1, int p2, int c_invalid, uint16_t *total,
                             void *stream);
int iamx_dense_sgm_paths(const uint8_t *volume, int width, int height, int planes, int paths, int p1,
                         int p2, int c_invalid, uint16_t *total, void *stream);
int iamx_dense_sgm_select(const uint16_t *total, const uint8_t *volume, int width, int height,
                          int planes, double w_far, double step, int max_cost, int32_t *plane,
                          uint8_t *cost, uint16_t *tot0, float *depth, void *stream);

/* ------------------------------------------------------------------------------------
 * Dense surface, coarse to fine (csrc/dense_refine.hip, the guided form in csrc/dense_sweep.hip): a
 * fine level sweeps, per tile, only a window of a larger set of planes around the depths that a
 * coarse depth map found.  The rules are stated in imageanalysis_amd/dense.py ("REFINEMENT RULES")
 * and restated in numpy by tests/dense_refine_restatement.py; the device follows them bit for bit.
 * All pointers DEV.
 *
 * windows [tiles_y][tiles_x][2] int32 = (first, count) per IAMX_DENSE_TILE_W x IAMX_DENSE_TILE_H tile
 * of the fine image, row-major, tiles_x = ceil(width / 32), tiles_y = ceil(height / 16); an entry
 * has 0 <= first, 0 <= count, first + count <= planes_total.  2 <= planes_total <=
 * IAMX_DENSE_GUIDED_MAX_PLANES planes uniform in inverse depth from w_far to w_near.
 *
 * iamx_dense_guide, one workgroup per tile: coarse_depth [hc][wc] float32 (NaN: none) -> windows.
 *   The tile grown by `radius` fine pixels maps to a box of coarse pixels (one more either side); the
 *   smallest and largest inverse depth of its finite positive entries, floor and ceil in fine plane
 *   steps, `pad` (0 .. IAMX_DENSE_GUIDED_MAX_PLANES) planes more either side, clamped into the set;
 *   (0, 0) for a box without an entry.  Every entry is written.
 * iamx_dense_sweep_guided: iamx_dense_sweep with planes_total in place of planes, and the tile's
 *   workgroup walking the planes of its window only; plane is the index in the whole set (-1 and NaN
 *   scores for a tile with count 0), around holds NaN beyond the window, and a winner on a rim of
 *   its window that is not a rim of the set has depth NaN.  The table is read back and checked before
 *   the launch (the stream is synchronised once); with every entry (0, planes_total) and
 *   planes_total <= IAMX_DENSE_MAX_PLANES the outputs are iamx_dense_sweep's.
 * A size or a parameter out of range, a null pointer, an entry that leaves the set: IAMX_EINVAL
 * without a launch.
 * ------------------------------------------------------------------------------------ */
#define IAMX_DENSE_GUIDED_MAX_PLANES 65536
int iamx_dense_guide(const float *coarse_depth, int wc, int hc, int width, int height, double w_far,
                     double w_near, int planes_total, int radius, int pad, int32_t *windows,
                     void *stream);
int iamx_dense_sweep_guided(const float *ref, const double *rays, const float *nbr,
                            const double *ref_pose, const double *nbr_cam, int width, int height,
                            int num_nbr, int planes_total, double w_far, double w_near, int radius,
                            float min_var, float min_score, const int32_t *windows, int32_t *plane,
                            float *score, float *depth, float *around, void *stream);

/* ------------------------------------------------------------------------------------
 * Dense surface, robust fusion (csrc/dense_fuse.hip): a DSM cell's height from the cluster of its
 * points that per-cell histograms find, in place of the mean of all of them.  The rules are stated
 * in imageanalysis_amd/dense.py ("ROBUST FUSION RULES") and restated in numpy by
 * tests/dense_fuse_restatement.py; the device follows them bit for bit.  All pointers DEV.
 *
 * ned, keep, num_points, x0, y1, gsd, width, height are iamx_dense_splat's, and so is the set of
 * accepted points: keep != 0, the cell inside the raster, q = rint(up 1024) with |q| <= 1e15.
 * window [H][W][2] int64 = (lo, hi) of a cell in units of q; hist [H][W][bins] uint32;
 * IAMX_DENSE_FUSE_MIN_BINS <= bins <= IAMX_DENSE_FUSE_MAX_BINS; wmin, the least bin width in units
 * of q, 1 .. 2^40; the bin width of a window is wb = max(wmin, ceil((hi - lo + 1) / bins)).
 *
 * iamx_dense_fuse_range, one thread per point: adds 1 to count [H][W] and takes the signed 64-bit
 *   atomic minimum / maximum of q into window; the caller starts count at 0 and every window at
 *   (INT64_MAX, INT64_MIN).
 * iamx_dense_fuse_hist, one thread per point: a point with lo <= q <= hi adds 1 to bin
 *   (q - lo) div wb of its cell; the caller zeroes hist before the first level only.
 * iamx_dense_fuse_select, 128 cells per workgroup: with s_b = hist[b-1] + hist[b] + hist[b+1] and
 *   smax their largest, b* = the highest b with s_b 256 >= share smax; window becomes
 *   (max(lo, lo + (b* - 1) wb), min(hi, lo + (b* + 2) wb - 1)), both from the old lo, and (0, 0) for
 *   a cell with count == 0; hist is left zeroed for the next level.  share 1 .. 256.  One level of
 *   the rule is hist then select; at most IAMX_DENSE_FUSE_MAX_LEVELS levels are meant to be chained.
 * iamx_dense_fuse_sum, one thread per point: a point with lo <= q <= hi adds 1 to support [H][W] and
 *   q to sum [H][W]; the caller zeroes both.  iamx_dense_resolve(support, sum) makes the DSM.
 * A size or a parameter out of range, a null pointer: IAMX_EINVAL without a launch; num_points == 0:
 * IAMX_OK without one (iamx_dense_fuse_select always launches).
 * ------------------------------------------------------------------------------------ */
#define IAMX_DENSE_FUSE_MIN_BINS 4
#define IAMX_DENSE_FUSE_MAX_BINS 64
#define IAMX_DENSE_FUSE_MAX_LEVELS 4
int iamx_dense_fuse_range(const double *ned, const uint8_t *keep, int64_t num_points, double x0,
                          double y1, double gsd, int width, int height, int32_t *count,
                          int64_t *window, void *stream);
int iamx_dense_fuse_hist(const double *ned, const uint8_t *keep, int64_t num_points, double x0,
                         double y1, double gsd, int width, int height, const int64_t *window,
                         int bins, int64_t wmin, uint32_t *hist, void *stream);
int iamx_dense_fuse_select(const int32_t *count, int width, int height, int bins, int64_t wmin,
                           int share, uint32_t *hist, int64_t *window, void *stream);
int iamx_dense_fuse_sum(const double *ned, const uint8_t *keep, int64_t num_points, double x0,
                        double y1, double gsd, int width, int height, const int64_t *window,
                        int32_t *support, int64_t *sum, void *stream);

/* ------------------------------------------------------------------------------------
 * True orthophoto (csrc/ortho_dsm.hip): a group's frames draped over the dense DSM, every mosaic
 * pixel placed at its DSM height, projected through the full camera model and coloured only from
 * the frames that see it.  The rules are stated in imageanalysis_amd/ortho.py ("THE TRUE-ORTHO
 * RULES") and the fill in imageanalysis_amd/dense.py; both are restated in numpy by
 * tests/ortho_dense_restatement.py and the device follows them bit for bit.  All pointers DEV
 * unless noted; null, size and range checks need no GPU.
 *
 * iamx_ortho_dsm_image, one image per launch, stream ordered -- the images of a group are composed
 *   in the order of the calls.  dsm [H][W] f32 (NaN: a hole); ss: the mosaic is H ss x W ss pixels,
 *   1 <= ss <= IAMX_ORTHO_DSM_MAX_UPSAMPLE, a side at most 2^20; params HOST f64
 *   [IAMX_ORTHO_DSM_PARAMS] = x0, y1, gsd (the DSM's frame), bias, zmax (the largest finite height),
 *   R[9] (NED -> camera, row-major), C[3] (NED), fx, fy, cx, cy at the frame's size, k1, k2, p1, p2,
 *   k3, all finite; frame u8 [h_s][w_s][3], at least 2 x 2; image_index: what `index` receives;
 *   c0, r0, c1, r1: the inclusive work box in mosaic pixels (c1 < c0 or r1 < r0: nothing is launched
 *   and the call succeeds).  mode, acc, index, count and bgr are iamx_ortho_raster_image's, over the
 *   mosaic: iamx_ortho_clear starts them and iamx_ortho_resolve finishes mode feather.
 * iamx_ortho_dsm_owner and iamx_ortho_dsm_layer, the two passes mode multiband's pyramid kernels
 *   (iamx_ortho_mb_reduce, _accumulate, _collapse) want over the dense surface; dsm, H, W, ss, params,
 *   h_s, w_s, image_index and the box are iamx_ortho_dsm_image's, and so are their checks.
 *   owner: mode best without frame and bgr -- count, metric f64 [H ss][W ss] and index exactly as
 *   iamx_ortho_dsm_image(mode 0) leaves count, acc and index; h_s, w_s: the size of the frame that
 *   will follow (the cover rule needs it, the pixels are not read).
 *   layer: no march.  layer f32 [r1 - r0 + 1][c1 - c0 + 1][4], 16-byte aligned, row-major over the
 *   box, iamx_ortho_mb_layer's layout = (C_b, C_g, C_r, A): C the bilinear sample (f64, cast to f32)
 *   wherever the image covers the pixel, seen or not, 0 elsewhere; A = 1 where index == image_index,
 *   else 0.  Every pixel of the box is written; index [H ss][W ss] is only read.
 * iamx_dense_fill, one round of the DSM hole fill per launch: round 0 copies src to dst and writes
 *   round_dst = 0 for a finite cell, 255 for an empty one (round_src is not read and may be NULL);
 *   round k = 1 .. 254 gives an empty cell with a finite value among its 8 neighbours of src their
 *   float32 sum in row-major order over their count (the quotient in float64, rounded once) and
 *   round_dst = k; every other cell and its round are copied.  src and dst are different rasters
 *   [height][width] f32, round_src and round_dst [height][width] u8.
 * A size or a parameter out of range, a null pointer, a box that leaves the mosaic: IAMX_EINVAL
 * without a launch.
 * ------------------------------------------------------------------------------------ */
#define IAMX_ORTHO_DSM_PARAMS 26
#define IAMX_ORTHO_DSM_MAX_UPSAMPLE 8
int iamx_ortho_dsm_image(int mode, const float *dsm, int H, int W, int ss, const double *params,
                         const uint8_t *frame, int h_s, int w_s, int image_index, int c0, int r0,
                         int c1, int r1, double *acc, int32_t *index, uint16_t *count, uint8_t *bgr,
                         void *stream);
int iamx_ortho_dsm_owner(const float *dsm, int H, int W, int ss, const double *params, int h_s,
                         int w_s, int image_index, int c0, int r0, int c1, int r1, double *metric,
                         int32_t *index, uint16_t *count, void *stream);
int iamx_ortho_dsm_layer(const float *dsm, int H, int W, int ss, const double *params,
                         const uint8_t *frame, int h_s, int w_s, int image_index, int c0, int r0,
                         int c1, int r1, const int32_t *index, float *layer, void *stream);
int iamx_dense_fill(const float *src, const uint8_t *round_src, int width, int height, int round,
                    float *dst, uint8_t *round_dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IAMX_H */
