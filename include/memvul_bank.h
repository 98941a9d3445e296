/* libmemvul_bank.so — the anchor-bank audit over a kept corpus: what a bank of vectors (the anchors, candidate anchors) decides AS A WHOLE once each vector has its
 * own threshold — the union decision and its multiplicity, each vector's sole claims (what deleting it loses), the pairwise overlap of the vectors' claims, and a
 * greedy cover (which candidate adds the most) — on one AMD GPU (gfx950).  Only integers leave the device.  A library of its own: nothing links against it and it
 * links against nothing of this tree.
 *
 * P(same) of a (row, vector) pair is, bit for bit, the fp32 value the engine's matcher produces for it (memvul_amd/csrc/bank_cover.h restates the arithmetic).
 * Vector q CLAIMS row n iff P(n, q) >= thres[q] in IEEE fp32: a NaN claims nothing.  Every result is an exact integer, and none depends on the plan (rows per block,
 * vectors per group, words per chunk), on first / count beyond the rows they select, or on how many mvb_add calls delivered the rows.
 *
 *   B[q][n]          the marking over rows [first, first + count): vector q claims row n
 *   claimed[q][c]    rows of class c with B[q][n]
 *   m[n]             sum over q of B[q][n]
 *   hist[c][j]       j = 0 .. Q: rows of class c with m[n] == j (hist[1][0]: the bank's false negatives; the sum over j >= 1: the union decision's TP / FP)
 *   sole[q][c]       rows of class c with B[q][n] and m[n] == 1: what deleting q loses
 *   overlap[q][r][c] rows of class c with B[q][n] and B[r][n]: symmetric, its diagonal is `claimed`
 *   greedy cover     vectors with fixed[q] != 0 are covered from the start and never picked; each round every other unpicked vector has
 *                    gain = w_pos * newpos - w_neg * newneg (int64; newpos / newneg: the rows of class 1 / 0 it claims that are not yet covered); the highest gain
 *                    wins, ties go to the lowest index; the loop stops before a pick whose gain is <= 0, after max_rounds picks, or when no candidate is left
 *
 * An index owns, on one device: the rows' embeddings U [N][P] in fp32, a per-row term, one class byte per row, the class-difference matcher weights, one stream,
 * its workspace, and the marking it holds.  One thread uses an index at a time.  Every int entry returns MVB_OK or an error code and leaves its output buffers
 * untouched on error; the text is read through mvb_last_error (NULL: the last mvb_create of this thread).  No C++ exception leaves the library.
 *
 * The held marking: a successful mvb_mark leaves B, the class words and the covered rows on the device.  mvb_totals, mvb_multiplicity, mvb_overlap, mvb_greedy,
 * mvb_count, mvb_kernel_ms and mvb_last_error read it as often as asked and leave it alone; EVERY other call on the index drops it when the call begins, whether
 * or not that call then succeeds (mvb_add, mvb_reset, mvb_set_classes, mvb_test_plan, and mvb_mark itself).  A reading call without a held marking returns
 * MVB_ERR_STATE.  count == 0 holds an empty marking: every reader returns zeros. */
#ifndef MEMVUL_BANK_H
#define MEMVUL_BANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVB_OK 0
#define MVB_ERR_ARG (-1)      /* a refused argument: a limit below, a NULL pointer */
#define MVB_ERR_HIP (-2)      /* the HIP runtime failed (no device, out of device memory, ...) */
#define MVB_ERR_NOMEM (-3)
#define MVB_ERR_INTERNAL (-4)
#define MVB_ERR_STATE (-5)    /* a reading call without a held marking */

#define MVB_MAX_VECTORS 4096         /* 1 <= Q <= 4096 */
#define MVB_MAX_ROWS 2147483646ll    /* N <= 2^31 - 2 */
#define MVB_MAX_WEIGHT (1 << 20)     /* mvb_greedy: 0 <= w_pos, w_neg <= 2^20 */
#define MVB_MAX_MARK_BYTES (4ll << 30) /* the held marking: 8 * Q * ceil(count / 64) bytes */

typedef struct mvb_index mvb_index;

/* proj_dim: 512 or 768.  Wm: the matcher weight, host fp32 [2][3 * proj_dim] (`_projector.weight`).  same_idx: 0 or 1. */
int mvb_create(int device, int proj_dim, const float* Wm, int same_idx, mvb_index** out);
void mvb_destroy(mvb_index* index);
const char* mvb_last_error(mvb_index* index);

/* host fp32 [n][proj_dim]; rows are numbered in order of arrival, their class is 0; capacity grows */
int mvb_add(mvb_index* index, const float* embed, int64_t n);
/* forget the rows (and their classes), keep the weights */
int mvb_reset(mvb_index* index);
int64_t mvb_count(mvb_index* index);
/* cls: host [n], the class (0 or 1) of rows [first, first + n).  A value above 1 is refused and changes nothing. */
int mvb_set_classes(mvb_index* index, const uint8_t* cls, int64_t first, int64_t n);

/* v: host fp32 [Q][proj_dim]; thres: host fp32 [Q], one finite threshold per vector.  Scores rows [first, first + count) and holds the marking on the device.  A
 * marking of more than MVB_MAX_MARK_BYTES is refused before anything is allocated (the message gives the figure). */
int mvb_mark(mvb_index* index, const float* v, int Q, const float* thres, int64_t first, int64_t count);
/* claimed [Q][2] */
int mvb_totals(mvb_index* index, int64_t* claimed);
/* hist [2][Q + 1], sole [Q][2]; mult uint16 [count] and sole_of int32 [count] (the one claimant where m == 1, otherwise -1): either may be NULL */
int mvb_multiplicity(mvb_index* index, int64_t* hist, int64_t* sole, uint16_t* mult, int32_t* sole_of);
/* overlap [Q][Q][2] */
int mvb_overlap(mvb_index* index, int64_t* overlap);
/* fixed: [Q] bytes or NULL (none).  max_rounds >= 0.  rounds: the number of picks; order [rounds] and gained [rounds][2] = (newpos, newneg) of each pick, in
 * buffers of min(max_rounds, Q) and 2 min(max_rounds, Q) entries */
int mvb_greedy(mvb_index* index, int64_t w_pos, int64_t w_neg, const uint8_t* fixed, int max_rounds, int* rounds, int32_t* order, int64_t* gained);
/* HIP-event time of the last call's launches (mvb_mark / mvb_totals / mvb_multiplicity / mvb_overlap / mvb_greedy over at least one row) */
int mvb_kernel_ms(mvb_index* index, float* ms);
/* tests only: rows per block of the scoring sweep (64, 128, 256, 512), vectors per group, words per chunk (multiplicity, overlap, greedy); 0 = the library's choice */
int mvb_test_plan(mvb_index* index, int block_rows, int vector_group, int word_chunk);

#ifdef __cplusplus
}
#endif
#endif
