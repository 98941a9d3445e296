/* libmemvul_rank.so — per-anchor ranking quality over a kept corpus: for every vector (an anchor of the bank, the embedding of a fresh CVE description) how well
 * its P(same) RANKS the rows of the corpus against their classes — the exact ROC-AUC, the average precision, and the threshold that maximises F1 over every
 * distinct score — on one AMD GPU (gfx950).  These are the three numbers the reference judges the matcher by (custom_metric.py:86-90, predict_memory.py:148-154),
 * per anchor and without the P(same) matrix ever leaving the device.  A library of its own: nothing links against it and it links against nothing of this tree.
 *
 * Inputs.  Rows [first, first + count) of the index, their class bytes (0 / 1), and Q vectors.
 * Scores.  P(row, q) is, bit for bit, the fp32 value the engine's matcher produces for the pair (memvul_amd/csrc/rank_sort.h restates the arithmetic).
 * NaN.     A row whose score for a vector is NaN is left out of that vector's ranking and counted in n_nan.
 * Sort key.  All other scores lie in [+0, 1], so their bit patterns order as the values do: key = bits << 1 | class fits 31 bits, and within a tie group it puts
 *          the negatives below the positives.
 * Tie groups.  For vector q let the distinct scores be t_1 > t_2 > ... (the tie groups, D of them); tp_g / fp_g are the positives / negatives with score exactly
 *          t_g, TP_g / FP_g those with score >= t_g.
 *
 * Outputs per vector:
 *   n[q]  = (n_neg, n_pos, n_nan), int64.
 *   u2[q] = sum_g tp_g * (2 * (n_neg - FP_g) + fp_g), int64: twice the Mann-Whitney U with ties at one half, an exact integer; AUC = u2 / (2 n_pos n_neg).
 *   ap[q] = sum_g (tp_g / n_pos) * (TP_g / (TP_g + FP_g)), float64 (sklearn's average_precision_score): every term is formed by two divisions and one product in
 *           float64; the terms are summed in a shape fixed by `count` alone (position p of the ascending order carries its group's term if it ends a group, else
 *           +0; 64 positions by a butterfly, four such sums left to right per 256 positions, the 256-blocks strided over 256 accumulators, those by a halving
 *           tree), so the BITS of ap depend on nothing in the plan.
 *   best_thres[q] (fp32, a score of the corpus) and best[q] = (TP, FP) at it: the distinct threshold maximising F1 = 2 TP / (TP + FP + n_pos) under the rule
 *           "claimed iff P >= thres"; fractions are compared exactly (128-bit cross products); a tie in F1 goes to the HIGHEST threshold, the side
 *           find_best_thres's `>=` over an ascending grid takes.
 * Degenerate cases.  n_pos == 0 (or count == 0): u2 = 0, ap = NaN, best_thres = NaN, best = (0, 0).  n_neg == 0: u2 = 0, the rest as defined.
 *
 * The bank slot (bank != 0 appends one result slot after the Q vectors): the row's score is the maximum over the Q vectors — what the reference itself measures
 * (s_auc, s_ave_precision_score, cal_metrics' auc / ap); a row with a NaN for any vector is left out and counted.
 *
 * Nothing in any result depends on the plan (rows per tile, vectors per group, workspace cap), on first / count beyond the rows they select, or on how many
 * mvk_add calls delivered the rows.
 *
 * An index owns, on one device: the rows' embeddings U [N][P] in fp32, a per-row term, one class byte per row, the class-difference matcher weights, one stream and
 * its workspace (bounded per group of vectors: RK_WORK_CAP_BYTES, rank_sort.h), and the curve it holds.  One thread uses an index at a time.  Every int entry
 * returns MVK_OK or an error code and leaves its output buffers untouched on error; the text is read through mvk_last_error (NULL: the last mvk_create of this
 * thread).  No C++ exception leaves the library.
 *
 * The held curve: a successful mvk_curve leaves its result on the device, and mvk_fetch copies it, as often as asked.  mvk_count, mvk_kernel_ms and
 * mvk_last_error leave it alone; EVERY other call on the index drops it when the call begins, whether or not that call then succeeds (mvk_add, mvk_reset,
 * mvk_set_classes, mvk_rank, mvk_test_plan, and mvk_curve itself).  mvk_fetch without a held curve is a state error. */
#ifndef MEMVUL_RANK_H
#define MEMVUL_RANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVK_OK 0
#define MVK_ERR_ARG (-1)      /* a refused argument: a limit below, a NULL pointer */
#define MVK_ERR_HIP (-2)      /* the HIP runtime failed (no device, out of device memory, ...) */
#define MVK_ERR_NOMEM (-3)
#define MVK_ERR_INTERNAL (-4)
#define MVK_ERR_STATE (-5)    /* mvk_fetch without a held curve */

#define MVK_MAX_VECTORS 4096           /* 1 <= Q <= 4096 */
#define MVK_MAX_ROWS 2147483646ll      /* N <= 2^31 - 2 rows in the index */
#define MVK_MAX_RANK_ROWS (1ll << 26)  /* count of one mvk_rank / mvk_curve call: one vector's workspace (13 bytes per row at the library's own tile) fits the default
                                          cap of 1 GiB, positions fit 32 bits, and u2 <= count^2 / 2 < 2^51 */

typedef struct mvk_index mvk_index;

/* proj_dim: 512 or 768.  Wm: the matcher weight, host fp32 [2][3 * proj_dim] (`_projector.weight`).  same_idx: 0 or 1. */
int mvk_create(int device, int proj_dim, const float* Wm, int same_idx, mvk_index** out);
void mvk_destroy(mvk_index* index);
const char* mvk_last_error(mvk_index* index);

/* host fp32 [n][proj_dim]; rows are numbered in order of arrival, their class is 0; capacity grows */
int mvk_add(mvk_index* index, const float* embed, int64_t n);
/* forget the rows (and their classes), keep the weights */
int mvk_reset(mvk_index* index);
int64_t mvk_count(mvk_index* index);
/* cls: host [n], the class (0 or 1) of rows [first, first + n).  A value above 1 is refused and changes nothing. */
int mvk_set_classes(mvk_index* index, const uint8_t* cls, int64_t first, int64_t n);

/* v: host fp32 [Q][proj_dim].  With S = Q + (bank ? 1 : 0) result slots: n [S][3], u2 [S], ap [S] (float64), best_thres [S] (fp32), best [S][2].  A count whose
 * single-vector workspace exceeds the cap is refused, with the figure in the message, before anything is allocated. */
int mvk_rank(mvk_index* index, const float* v, int Q, int bank, int64_t first, int64_t count, int64_t* n, int64_t* u2, double* ap, float* best_thres, int64_t* best);
/* the whole curve of ONE ranking: bank == 0 requires Q == 1; bank != 0 takes the bank score of the Q vectors.  The result stays on the device: *points tie groups,
 * thres descending, with TP_g and FP_g — the data of roc_curve(drop_intermediate=False) and precision_recall_curve. */
int mvk_curve(mvk_index* index, const float* v, int Q, int bank, int64_t first, int64_t count, int64_t* points);
/* the held curve: thres [points] (fp32, descending), tp [points], fp [points] */
int mvk_fetch(mvk_index* index, float* thres, int64_t* tp, int64_t* fp);
/* HIP-event time of the last call's launches (mvk_rank / mvk_curve over at least one row): ms [4] = the whole, and its score, sort and statistics stages */
int mvk_kernel_ms(mvk_index* index, float* ms);
/* tests only: rows per sort tile (256, 512, 1024), vectors per group, the workspace cap in bytes; 0 = the library's own choice */
int mvk_test_plan(mvk_index* index, int tile_rows, int vector_group, int64_t work_cap_bytes);

#ifdef __cplusplus
}
#endif
#endif
