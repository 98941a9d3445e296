/* libmemvul_retrieve.so — per-anchor retrieval over a kept corpus: for every query vector (an anchor of the bank, the embedding of a fresh CVE description) the k rows
 * of the corpus with the highest P(same), on one AMD GPU (gfx950).  The other direction of libmemvul_hip.so's match (which anchors fit a report); a library of
 * its own, which libmemvul_hip.so does not link against.
 *
 * P(same) of a (row, vector) pair is, bit for bit, the fp32 value the engine's matcher produces for it (memvul_amd/csrc/report_topk.h restates the arithmetic); the
 * ranking per vector is (key(P) descending, row ascending) with key(NaN) = 2.0.  Nothing in a result depends on the plan (rows per block, lists per merge, vectors
 * per group), on first / count beyond the rows they select, or on how many mvr_add calls delivered the rows.
 *
 * An index owns, on one device: the rows' embeddings U [N][P] in fp32, a per-row term, the class-difference matcher weights, one stream and its workspace (the
 * candidate lists are bounded: RT_LIST_CAP_BYTES, report_topk.h).  One thread uses an index at a time.  Every int entry returns MVR_OK or an error code and
 * leaves its output buffers untouched on error; the text is read through mvr_last_error (NULL: the last mvr_create of this thread).  No C++ exception leaves the
 * library. */
#ifndef MEMVUL_RETRIEVE_H
#define MEMVUL_RETRIEVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVR_OK 0
#define MVR_ERR_ARG (-1)      /* a refused argument: a limit below, a NULL pointer */
#define MVR_ERR_HIP (-2)      /* the HIP runtime failed (no device, out of device memory, ...) */
#define MVR_ERR_NOMEM (-3)
#define MVR_ERR_INTERNAL (-4)

#define MVR_MAX_K 64                 /* 1 <= k <= 64 */
#define MVR_MAX_QUERIES 4096         /* 1 <= Q <= 4096 */
#define MVR_MAX_ROWS 2147483646ll    /* N <= 2^31 - 2 */
#define MVR_MAX_PSAME (1ll << 28)    /* mvr_psame: count * Q values per call */

typedef struct mvr_index mvr_index;

/* proj_dim: 512 or 768.  Wm: the matcher weight, host fp32 [2][3 * proj_dim] (`_projector.weight`).  same_idx: 0 or 1. */
int mvr_create(int device, int proj_dim, const float* Wm, int same_idx, mvr_index** out);
void mvr_destroy(mvr_index* index);
const char* mvr_last_error(mvr_index* index);

/* host fp32 [n][proj_dim]; rows are numbered in order of arrival; capacity grows */
int mvr_add(mvr_index* index, const float* embed, int64_t n);
/* forget the rows, keep the weights */
int mvr_reset(mvr_index* index);
int64_t mvr_count(mvr_index* index);

/* v: host fp32 [Q][proj_dim].  Ranks rows [first, first + count): top_p [Q][k], top_row [Q][k] (row numbers of the index).  A query over zero rows, or k beyond
 * the rows in range: the exhausted slots hold p = -1, row = -1. */
int mvr_query(mvr_index* index, const float* v, int Q, int k, int64_t first, int64_t count, float* top_p, int64_t* top_row);
/* P(same) of rows [first, first + count) against every vector: p [count][Q]; count * Q <= 2^28 */
int mvr_psame(mvr_index* index, const float* v, int Q, int64_t first, int64_t count, float* p);
/* HIP-event time of the last query's launches (mvr_query / mvr_psame over at least one row) */
int mvr_kernel_ms(mvr_index* index, float* ms);
/* tests only: rows per block (64, 128, 256, 512), lists per merge (2 .. 16), query vectors per group; 0 = the library's own choice */
int mvr_test_plan(mvr_index* index, int block_rows, int fan_in, int anchor_group);

#ifdef __cplusplus
}
#endif
#endif
