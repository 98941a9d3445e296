/* libmemvul_claims.so — per-anchor claims over a kept corpus: for every vector (an anchor of the bank, the embedding of a fresh CVE description) EVERY row of the
 * corpus whose P(same) reaches a threshold, and per vector and threshold the number of rows of each class it claims, on one AMD GPU (gfx950).  The reference decides
 * by a threshold (prob >= thres), not by a rank; this library answers by that rule.  A library of its own: nothing links against it and it links against nothing
 * of this tree.
 *
 * P(same) of a (row, vector) pair is, bit for bit, the fp32 value the engine's matcher produces for it (memvul_amd/csrc/claim_sweep.h restates the arithmetic).  A
 * pair is CLAIMED iff P(same) >= t in IEEE fp32: a NaN claims nothing.  Nothing in a result depends on the plan (rows per block, vectors per group), on first /
 * count beyond the rows they select, or on how many mvc_add calls delivered the rows.
 *
 * An index owns, on one device: the rows' embeddings U [N][P] in fp32, a per-row term, one class byte per row, the class-difference matcher weights, one stream and
 * its workspace (bounded per group of vectors: CL_WORK_CAP_BYTES, claim_sweep.h), and the selection it holds.  One thread uses an index at a time.  Every int entry
 * returns MVC_OK or an error code and leaves its output buffers untouched on error; the text is read through mvc_last_error (NULL: the last mvc_create of this
 * thread).  No C++ exception leaves the library.
 *
 * The held selection: a successful mvc_select leaves its result on the device, and mvc_fetch copies it, as often as asked.  mvc_count, mvc_kernel_ms and
 * mvc_last_error leave it alone; EVERY other call on the index drops it when the call begins, whether or not that call then succeeds (mvc_add, mvc_reset,
 * mvc_set_classes, mvc_counts, mvc_test_plan, and mvc_select itself).  mvc_fetch without a held selection is a state error. */
#ifndef MEMVUL_CLAIMS_H
#define MEMVUL_CLAIMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVC_OK 0
#define MVC_ERR_ARG (-1)      /* a refused argument: a limit below, a NULL pointer */
#define MVC_ERR_HIP (-2)      /* the HIP runtime failed (no device, out of device memory, ...) */
#define MVC_ERR_NOMEM (-3)
#define MVC_ERR_INTERNAL (-4)
#define MVC_ERR_STATE (-5)    /* mvc_fetch without a held selection */

#define MVC_MAX_THRESHOLDS 64        /* mvc_counts: 1 <= T <= 64 */
#define MVC_MAX_VECTORS 4096         /* 1 <= Q <= 4096 */
#define MVC_MAX_ROWS 2147483646ll    /* N <= 2^31 - 2 */
#define MVC_MAX_PAIRS (1ll << 28)    /* mvc_select: claimed pairs per call */

typedef struct mvc_index mvc_index;

/* proj_dim: 512 or 768.  Wm: the matcher weight, host fp32 [2][3 * proj_dim] (`_projector.weight`).  same_idx: 0 or 1. */
int mvc_create(int device, int proj_dim, const float* Wm, int same_idx, mvc_index** out);
void mvc_destroy(mvc_index* index);
const char* mvc_last_error(mvc_index* index);

/* host fp32 [n][proj_dim]; rows are numbered in order of arrival, their class is 0; capacity grows */
int mvc_add(mvc_index* index, const float* embed, int64_t n);
/* forget the rows (and their classes), keep the weights */
int mvc_reset(mvc_index* index);
int64_t mvc_count(mvc_index* index);
/* cls: host [n], the class (0 or 1) of rows [first, first + n).  A value above 1 is refused and changes nothing. */
int mvc_set_classes(mvc_index* index, const uint8_t* cls, int64_t first, int64_t n);

/* v: host fp32 [Q][proj_dim]; thres: host fp32 [T], finite, in any order, duplicates allowed.  counts [Q][T][2]: counts[q][t][c] = the rows of class c among
 * [first, first + count) with P(row, q) >= thres[t]. */
int mvc_counts(mvc_index* index, const float* v, int Q, const float* thres, int T, int64_t first, int64_t count, int64_t* counts);
/* thres: host fp32 [Q], one finite threshold per vector.  Scores, marks and compacts on the device; offsets [Q + 1]: vector q claims offsets[q + 1] - offsets[q]
 * rows of [first, first + count).  More than 2^28 claimed pairs are refused before anything is allocated for them (the message gives the total). */
int mvc_select(mvc_index* index, const float* v, int Q, const float* thres, int64_t first, int64_t count, int64_t* offsets);
/* the held selection: rows [offsets[Q]] (row numbers of the index, ascending within a vector) and p [offsets[Q]], each row's P(same) */
int mvc_fetch(mvc_index* index, int64_t* rows, float* p);
/* HIP-event time of the last call's launches (mvc_counts / mvc_select over at least one row) */
int mvc_kernel_ms(mvc_index* index, float* ms);
/* tests only: rows per block (64, 128, 256, 512), vectors per group; 0 = the library's own choice */
int mvc_test_plan(mvc_index* index, int block_rows, int vector_group);

#ifdef __cplusplus
}
#endif
#endif
