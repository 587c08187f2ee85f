/*
 * colbert_mi355x.h — C ABI of libcolbert_mi355x.so, the MI355X (gfx950) ColBERT
 * late-interaction scoring path.
 *
 * The reference (techmum21p/hybrid-rag-ColBERTv2) has no FFI: its seam is the
 * Python object `DualIndexer.colbert_retriever` (local_rag_complete.py:844)
 * called as `.search(query=, k=)` (:954) and `.rerank(query=, documents=, k=)`
 * (:999).  Each entry point below replaces one piece of arithmetic behind that
 * seam; the Python package (hybrid-rag-colbertv2_amd/) binds them with ctypes
 * and keeps the reference's method names and result dicts.
 *
 * Conventions
 *  - Every pointer argument except `cbv2_index*` is a DEVICE pointer owned by
 *    the caller (torch tensors in the Python layer), except where a
 *    declaration says HOST: the host-only helpers (cbv2_rrf_fuse, BM25, the
 *    index file, the stemmer) and the stage-1 lists / host stage of
 *    cbv2_retrieve_finish.  Nothing is allocated or freed inside a compute
 *    call.
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = legacy default
 *    stream).  One index handle belongs to one device.
 *  - Batch sizes.  B is the number of queries (rows) of a call, an int32.
 *    Bounded, B in [1, 65535] (B = 65536 returns CBV2_EINVAL, launches
 *    nothing and writes nothing):
 *      every call that takes f32 queries on an fp32-faithful index:
 *      cbv2_score_f32, cbv2_search_f32, cbv2_search_f32_begin / _finish,
 *      cbv2_rerank_f32, cbv2_search_filtered_f32, cbv2_search_grouped_f32,
 *      and cbv2_search_filtered / cbv2_search_filtered_batch /
 *      cbv2_search_grouped when q_dtype is CBV2_DTYPE_F32 on such an index;
 *      cbv2_filter_batch_create, and through its batch -- B must equal the
 *      batch's -- every cbv2_search_filtered_batch.
 *      It is the CALL that rejects.  Of the size functions only
 *      cbv2_filter_batch_bytes and cbv2_search_grouped_f32_workspace_size
 *      return 0 for B > 65535; the others (cbv2_f32_workspace_bytes,
 *      cbv2_search_filtered*_workspace_size,
 *      cbv2_search_grouped_workspace_size) answer for any B >= 1, also
 *      where the call would reject it.
 *    Unbounded, B >= 1 (as far as the buffers and the workspace fit memory):
 *      cbv2_score, cbv2_search, cbv2_rerank, cbv2_rerank_ws, and with bf16 or
 *      MXFP8 queries cbv2_search_filtered and cbv2_search_grouped;
 *      cbv2_select_topk, cbv2_topk_rows, cbv2_merge_topk,
 *      cbv2_group_topk_rows.
 *    cbv2_retrieve_begin / _finish take the bound of the search they run:
 *      B >= 1 on a bf16 or MXFP8 index, B in [1, 65535] on an fp32-faithful
 *      one (cbv2_search_f32 inside begin returns the CBV2_EINVAL).
 *    Results do not depend on B: above 64 query groups of a scan launch
 *    (B > 2048 for bf16, 4096 for MXFP8) the dynamic tail gives way to the
 *    static split unless CBV2_OPT_DYNAMIC_TAIL = 2, and with more query
 *    groups than resident workgroups one chunk spans the shard; the scores
 *    are the same bit for bit.  tests/test_gpu_bigbatch.py runs every entry
 *    point on both sides of each of these points, at 65535 (retrieve up to
 *    2049), the bounded calls at 65536, and the unbounded selection, score,
 *    filtered and grouped calls at 65536 and 70001.
 *  - hipGraph capture.  These calls may be issued on a capturing stream, and
 *    every replay of the graph recomputes them from the buffers' contents at
 *    replay time (tests/test_gpu_graph_replay.py replays each of them over
 *    poisoned workspaces and outputs):
 *      cbv2_score, cbv2_score_f32, cbv2_quantize_mxfp8,
 *      cbv2_search, cbv2_search_f32, cbv2_search_filtered (the filter created
 *      before the capture),
 *      cbv2_rerank, cbv2_rerank_ws, cbv2_rerank_f32,
 *      cbv2_select_topk, cbv2_topk_rows, cbv2_merge_topk, cbv2_split_f32.
 *    A replay re-initialises every counter and flag it uses in the caller's
 *    workspace; a graph and the eager calls between its replays may share a
 *    handle and, on one stream, a workspace.  What the handle itself owns per
 *    launch stays out of a capture:
 *      - a capturing cbv2_score takes no slot of the handle's task-counter
 *        ring and runs the static work split, without the dynamic tail (the
 *        scores are the same bit for bit; searches keep their tail: their
 *        counters are in the caller's workspace);
 *      - with cbv2_index_time_scans enabled, launches on a capturing stream
 *        are not timed: cbv2_index_scan_times / _band_times report the eager
 *        launches only, never a graph's replays.
 *    The list above has one more member, cbv2_search_filtered_batch (the
 *    per-query form of cbv2_search_filtered; the filter batch created before
 *    the capture): it may be issued on a capturing stream, every replay
 *    recomputes it from the buffers' contents at replay time and
 *    re-initialises what it uses in the caller's workspace, like the searches
 *    above (tests/test_gpu_filter_batch.py replays it over a poisoned
 *    workspace and poisoned outputs).
 *    So has cbv2_search_filtered_f32 (the filter created before the capture;
 *    tests/test_gpu_filter_band.py replays it the same way).
 *    Outside the list, not to be captured: cbv2_retrieve_* (pooled mapped buffers, a second stream
 *    and host polling), the sharded and loopback calls, cbv2_filter_create
 *    (waits for its count), cbv2_filter_batch_create (copies its table from
 *    the host and waits for it), the index-file, writer and cbv2_hbm_* calls, and
 *    cbv2_index_build_means.
 *  - Return 0 on success, a negative CBV2_E* code on error; the message is in
 *    the thread-local `cbv2_last_error()`.  Arguments are validated on the host
 *    BEFORE any launch: a call that returns an error has launched nothing.
 *  - Bounds.  No call writes outside the extents stated in this file (an
 *    output [B][k], a workspace of exactly its *_workspace_size bytes, a
 *    filter `buf` of exactly cbv2_filter_bytes(n) bytes), no value outside
 *    them influences a result (doc n, doclens[n], bitmap bits at or past n,
 *    candidate C), and inputs are never written.  Pinned by
 *    tests/test_gpu_bounds.py, which runs every device entry point inside
 *    guard bands.
 *  - Sizes.  Index arrays (tokens, residual) and score matrices larger than
 *    4 GiB are supported by every entry point, caller-given row strides
 *    (ld_out, ld) past 2^31 elements included; pinned by
 *    tests/test_gpu_high_offsets.py, which runs every index path on docs
 *    astride byte offsets 2^31 and 2^32 of the token arrays.
 *  - Ranking ties are broken deterministically: score descending, then the
 *    lower index in the scored list (doc id for search, candidate position for
 *    rerank).  The reference's torch.topk / argsort (local_rag_complete.py:767,
 *    :789) leave tie order unspecified; this is the defined refinement.
 *    "Score descending" is the order of the scores' order-preserving bit keys
 *    in every selection (search, rerank, select, merge, groups): -0.0 ranks
 *    below +0.0, the two are no tie; NaN scores are undefined.
 *
 * Index layout in HBM (see DESIGN.md "Data layout"):
 *    tokens   bf16 [n][ld][d = 128], row-major, 16-byte aligned; ld = 128
 *             token slots (every path), or 256 / 512 / 1024 for long
 *             documents (bf16 and MXFP8 MaxSim scan, search and rerank, the
 *             fp32-faithful index and the native file; scales of an MXFP8
 *             index are [n][ld][2]);
 *             rows t >= doclens[i] of doc i are padding and never score.
 *             Padding rows -- of the tokens, of the residual of an
 *             fp32-faithful index, of the f32 source matrix of the index
 *             split and of the mean build, and for MXFP8 their scale bytes
 *             -- may hold ANY bit pattern, NaN and Inf encodings included (an
 *             allocation never cleared, a 0xFF byte fill): no result depends
 *             on them (tests/test_gpu_nonfinite_padding.py).
 *    doclens  int32 [n], 0 <= doclens[i] <= ld.
 *    Local doc i has global id  id_base + i  (contiguous shard of the corpus).
 */
#ifndef COLBERT_MI355X_H
#define COLBERT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBV2_ABI_VERSION 2

/* dtypes */
#define CBV2_DTYPE_BF16 1
#define CBV2_DTYPE_F32 2
#define CBV2_DTYPE_MXFP8 3 /* e4m3 bytes + one E8M0 scale per token per 64 dims */

/* scorers */
#define CBV2_SCORER_MAXSIM 0              /* sum_i max_j <q_i, d_j>            */
#define CBV2_SCORER_REF_MEANPOOL_COSINE 1 /* cos(mean_i q_i, mean_j d_j)       */

/* error codes */
#define CBV2_OK 0
#define CBV2_EINVAL -1       /* bad argument (shape, null pointer, range)       */
#define CBV2_EUNSUPPORTED -2 /* valid but not built (e.g. ld != 128)             */
#define CBV2_EHIP -3         /* a HIP runtime call failed                        */
#define CBV2_ESTATE -4       /* handle not ready (e.g. meanpool means not built) */

typedef struct cbv2_index cbv2_index;

/* Library / error reporting ------------------------------------------------ */
int cbv2_abi_version(void);
const char* cbv2_last_error(void);
/* "cbv2-build-stamp:<hex>": a content hash of the sources and compiler flags
 * the library was built from (build provenance; the Python loader refuses a
 * library whose stamp differs from the tree's sources).                     */
const char* cbv2_build_stamp(void);

/* Index handle --------------------------------------------------------------
 * Replaces the tensor the reference keeps in `self.corpus_embeddings`
 * (local_rag_complete.py:735-739 index(), :751-752 load()).  The handle
 * BORROWS `tokens`, `doclens` (and later `doc_means`): the caller keeps them
 * alive until cbv2_index_destroy.  `device` is the HIP device ordinal.      */
int cbv2_index_create(int device, const void* tokens, int32_t dtype, int64_t n, int32_t ld,
                      int32_t d, const int32_t* doclens, int64_t id_base, cbv2_index** out);
int cbv2_index_destroy(cbv2_index* index);

/* Index memory placement (no reference counterpart).  cbv2_hbm_alloc: `bytes`
 * of device memory on `device`, PHYSICALLY CONTIGUOUS when the driver can
 * provide it (hipExtMallocWithFlags(hipDeviceMallocContiguous); *contiguous =
 * 1), else plain hipMalloc (0).  Large index buffers (the token arrays every
 * scan streams) belong there: the B = 1 streaming scan over 1M docs (32.8 GB)
 * ran 4.63-4.67 ms from contiguous allocations and 4.75-4.99 ms from plain
 * hipMalloc ones of the same process (tools/probes/alloc_probe.cpp) -- the
 * translation of a streamed range is cheaper when it is one contiguous
 * physical range.  Free with cbv2_hbm_free (synchronous, like hipFree).    */
int cbv2_hbm_alloc(int device, size_t bytes, void** out, int32_t* contiguous);
int cbv2_hbm_free(int device, void* p);

/* Scan timing (measurement only; no reference counterpart -- the reference
 * prints wall-clock stage timings, local_rag_complete.py:905-933).  While
 * enabled, every MaxSim scan launch of this handle (cbv2_score / cbv2_search /
 * cbv2_search_f32) is bracketed by HIP events recorded on the launch's own
 * stream, so a benchmark can time the dominant kernel inside its timed region
 * without a side launch.  enable=1 clears the previous record.  Launches on
 * a stream that is capturing a hipGraph are not timed (Conventions).
 * cbv2_index_scan_times (timing disabled first) waits for the recorded launches
 * and writes min(count, max) durations in ms; *count = launches recorded;
 * the record is then cleared.
 * cbv2_index_band_times: the same for the fp32-faithful searches' band work
 * (cbv2_search_f32 / _begin + _finish), each bracketed from the end of the
 * bf16 top-k of its scan to the end of its band select and full-scan fallback:
 * the time the faithful arithmetic adds to a bf16 search (the query split
 * before the scan, one small kernel, is outside the bracket).
 * enable=2: the events, plus the clock probe of the doc-interleaved scans
 * (bf16 maxsim_scan16x4_kernel, MXFP8 maxsim_scan_f8x4_kernel): each of their
 * workgroups adds its run time in shader cycles (s_memtime) and in 10-ns ticks
 * (s_memrealtime) to the handle's sums.  cbv2_index_scan_clock (after the
 * launches completed) writes out4 = {sum of cycles, sum of ticks, workgroups
 * started, workgroups ended} since enable=2 or the last reset (reset != 0
 * zeroes them after the read): the clock the scans held in THIS run is
 * out4[0] / out4[1] x 0.1 GHz.  */
int cbv2_index_time_scans(cbv2_index* index, int32_t enable);
int cbv2_index_scan_times(cbv2_index* index, float* ms, int32_t max, int32_t* count);
int cbv2_index_band_times(cbv2_index* index, float* ms, int32_t max, int32_t* count);
int cbv2_index_scan_clock(cbv2_index* index, int64_t* out4, int32_t reset);

/* Handle options (A/B and tests; defaults = production):
 *  CBV2_OPT_FUSED_TOPK   1: cbv2_search fuses the top-k into eligible scans
 *                        (the bf16 doc-interleaved scan; 2 the same -- the
 *                        fused MXFP8 scan spills and is built in lab builds
 *                        only).  Default 0: on MI355X the fused scan runs
 *                        ~1 % longer than the scan + radix top-k.
 *  CBV2_OPT_DYNAMIC_TAIL 1: large scans hand the last part of the corpus out
 *                        as dynamic tasks, in 8 XCD-local slices (2: one
 *                        shared tail; 0: static chunks only).
 *  CBV2_OPT_BAND_DOC_MAJOR 0 (default): cbv2_search_f32 rescores the band
 *                        pair by pair (one (query, doc) pair per workgroup);
 *                        1-4: a batch of more than 8 queries grouped by doc
 *                        (each band doc read once per batch) -- 1 one wave
 *                        per doc, its halves in turn; 2 the same, pair-outer;
 *                        3 / 4 one doc per workgroup of 4 / 2 waves (128-slot
 *                        docs; others take 1).  Identical results either way.
 *  CBV2_OPT_BAND_LOWER_BOUND 1: cbv2_search_f32 first rescores the bf16
 *                        top-k, whose minimum faithful score lb bounds the
 *                        k-th from below, and bands T >= lb - beta (0: the
 *                        wider T >= T_k - 2 beta).  Identical results.
 *  CBV2_OPT_BAND_FUSED   1: cbv2_search_f32 on at most 8 queries (128-slot
 *                        docs) collects the band and rescores it in ONE
 *                        launch (0: a collect launch, then a rescoring
 *                        launch).  Identical results.
 *  CBV2_OPT_RESCORE_SPLIT 1: the fp32-faithful rescorings (the bf16 top-k, the
 *                        band of <= 8 queries, rerank candidates, the
 *                        full-scan fallback) score one (query, doc) pair per
 *                        workgroup, the doc's rows split over its 4 waves (0:
 *                        one pair per wave).  Identical results.
 *  CBV2_OPT_BAND_REUSE   1: the two-pass band of cbv2_search_f32 keeps the
 *                        faithful scores phase 1 computed for the bf16 top-k
 *                        (its lower bound) as its first k entries and rescores
 *                        only the rest (0: the whole band).  Needs
 *                        CBV2_OPT_RESCORE_SPLIT.  Identical results.
 *  CBV2_OPT_BAND_BLOCK_SKIP 1: the band collect of cbv2_search_f32 reads only
 *                        the 64-doc blocks whose maximum (left by the
 *                        block-max top-k) reaches the band threshold (0: the
 *                        whole score row).  Identical results.
 *  CBV2_OPT_RESCORE_GRID  workgroups per row of a split rescoring launch (0:
 *                        automatic, 4096 / B within [256, 1024]; rows with
 *                        more pairs grid-stride).
 *                        Identical results.
 *  CBV2_OPT_DENSE_DOCS    1: the docs fill (nearly) all 128 token slots, so
 *                        searches of B <= 2 stream every slot on the 4-wave
 *                        x 1-query scan (non-temporal) instead of the
 *                        streaming scan that skips empty 16-token tiles
 *                        (0, the default; the Python ColbertIndex sets it
 *                        when >= 98 % of the tiles hold tokens).  Identical
 *                        results.
 *  CBV2_OPT_TOPK_BMAX    1: cbv2_search's unfused MaxSim scan (rows of >= 65,536
 *                        and <= 1,572,864 docs, k <= 1024) also folds the max of
 *                        every 64-doc block, and ONE select launch reads only
 *                        the blocks that can reach the top-k (0: the sampled
 *                        filter + select).  Identical results.
 *  CBV2_OPT_P1_COLLECT_FUSED 1: the two-pass band of cbv2_search_f32 on at
 *                        most 8 queries runs its phase 1 (the bf16 top-k's
 *                        faithful scores) and the band collect in ONE launch
 *                        (the collect's loads overlap phase 1; 0: two
 *                        launches).  Identical results.
 *  CBV2_OPT_FOLD_KEYS     1: cbv2_search_f32 on at most 4 queries of a
 *                        dense-doc index folds the block-max select's block
 *                        keys into its 4 x 1 scan (atomic max into keys the
 *                        query split zeroes; 0: a pass over the scores).
 *                        Identical results.
 *  CBV2_OPT_FILTER_PATH   cbv2_search_filtered's path: 0 automatic (the subset
 *                        path where it is supported and m <= 0.5 n, the
 *                        largest measured density at which it still beat the
 *                        dense path, for bf16, fp32-faithful and MXFP8
 *                        indexes alike, of 128-slot docs (measured at 1M
 *                        docs) and of long documents (measured at ld = 256,
 *                        512 and 1024, 32 GB of bf16 tokens each): DESIGN.md
 *                        3.8), 1 the subset path where
 *                        supported (MaxSim, every index kind and ld), 2 the
 *                        dense path (score every doc, gather the allowed
 *                        columns).  Identical results.
 *  CBV2_OPT_FILTER_BAND   the filtered faithful search (cbv2_search_filtered_f32,
 *                        cbv2_search_filtered with f32 queries) where
 *                        CBV2_OPT_FILTER_PATH resolves to the subset path: 0
 *                        automatic (a rule of B, m and k), 1 the
 *                        band over the compact row wherever it is supported
 *                        (m > k, k <= 16384), 2 never (one faithful score per
 *                        (query, allowed doc)).  Identical results.
 *  CBV2_OPT_GROUP_BAND    the grouped faithful search (cbv2_search_grouped_f32,
 *                        cbv2_search_grouped with f32 queries on a faithful
 *                        index): 0 automatic (a rule of B, n, k, r and the
 *                        groups per k), 1 the certified band wherever
 *                        it is supported (G' > k, k <= 16384, k r <= cap,
 *                        CBV2_OPT_RESCORE_SPLIT on), 2 never (the full faithful
 *                        scan of every chunk).  Identical results.
 *  CBV2_OPT_FILTER_BATCH_CHUNK_DOCS  docs per work item of the per-query
 *                        filters' ragged scan (0: automatic, from the batch's
 *                        pair count and the CU count; > 0: for tests).  Read
 *                        by cbv2_filter_batch_create.  Identical results.
 * cbv2_index_last_scan_plan: the work split of this handle's latest scan
 * launch: {workgroups, static chunk docs, static docs, dynamic tail 0/1}.
 * Thread safety: one handle may be used from several host threads and
 * streams; the options and the last plan are plain fields (set options
 * before sharing the handle).                                               */
#define CBV2_OPT_FUSED_TOPK 1
#define CBV2_OPT_DYNAMIC_TAIL 2
#define CBV2_OPT_BAND_DOC_MAJOR 3
#define CBV2_OPT_BAND_LOWER_BOUND 4
#define CBV2_OPT_TOPK_BMAX 5
#define CBV2_OPT_BAND_FUSED 6
#define CBV2_OPT_RESCORE_SPLIT 7
#define CBV2_OPT_BAND_REUSE 8
#define CBV2_OPT_BAND_BLOCK_SKIP 9
#define CBV2_OPT_RESCORE_GRID 10
#define CBV2_OPT_DENSE_DOCS 11
#define CBV2_OPT_P1_COLLECT_FUSED 12
#define CBV2_OPT_FOLD_KEYS 13
#define CBV2_OPT_FILTER_PATH 14
#define CBV2_OPT_FILTER_BATCH_CHUNK_DOCS 15
#define CBV2_OPT_FILTER_BAND 16
#define CBV2_OPT_GROUP_BAND 17
int cbv2_index_set_option(cbv2_index* index, int32_t option, int64_t value);
int cbv2_index_last_scan_plan(const cbv2_index* index, int64_t* out4);
/* Per-query workgroup lists a cbv2_search of (B, k, scorer) keeps with the
 * top-k fused into the scan; 0 = that search runs unfused.                  */
int64_t cbv2_search_fused_slots(const cbv2_index* index, int32_t B, int32_t k, int32_t scorer);

/* MXFP8 index (config 5: half the HBM bytes of bf16, scored on the
 * block-scaled fp8 MFMA): tokens e4m3 [n][128][128] (16-B aligned), scales
 * E8M0 [n][128][2] (byte h scales dims 64h .. 64h+63 by 2^(byte-127)).
 * Queries for such an index are MXFP8 too (q_dtype CBV2_DTYPE_MXFP8): one
 * buffer holding B*lq*128 e4m3 bytes followed by B*lq*2 scale bytes, as
 * written by cbv2_quantize_mxfp8 (rows = B*lq, scales = q + rows*128).     */
int cbv2_index_create_mxfp8(int device, const void* tokens, const void* scales, int64_t n, int32_t ld,
                            int32_t d, const int32_t* doclens, int64_t id_base, cbv2_index** out);

/* cbv2_quantize_mxfp8 — rows of 128 values (dtype BF16 or F32) -> e4m3 bytes
 * q [rows][128] (round-to-nearest-even) and E8M0 scales [rows][2], with
 * scale = the smallest power of two that keeps each 64-value half <= 448.   */
int cbv2_quantize_mxfp8(const void* x, int32_t dtype, int64_t rows, void* q, void* scales, void* stream);

/* Literal-reference scorer support: build the L2-normalised per-doc token means
 * the reference recomputes on every call (local_rag_complete.py:822,825-829)
 * ONCE, from the fp32 encoder output `tokens_f32` [n][ld_src][d].
 * `doc_means` is a caller-owned f32 [n][d] buffer the handle borrows.        */
int cbv2_index_build_means(cbv2_index* index, const float* tokens_f32, int32_t ld_src,
                           float* doc_means, void* stream);

/* Scoring -------------------------------------------------------------------
 * cbv2_score — JinaColBERTRetriever._maxsim_score (local_rag_complete.py:802-831)
 * for a batch of B queries against every doc of the index:
 *    out[b * ld_out + i] = score(Q[b], doc i)     (i = local index)
 *  scorer MAXSIM:              Q bf16 [B][lq][128], 1 <= lq <= 32.
 *  scorer REF_MEANPOOL_COSINE: Q f32  [B][lq][128], any lq >= 1 (means must
 *                              be built).                                    */
int cbv2_score(cbv2_index* index, int32_t scorer, const void* Q, int32_t q_dtype, int32_t B,
               int32_t lq, float* out, int64_t ld_out, void* stream);

/* cbv2_search — JinaColBERTRetriever.search (local_rag_complete.py:755-777):
 * score every doc, then top-k (torch.topk at :767) with the deterministic tie
 * rule.  Writes out_scores f32 [B][k] and out_ids int32 [B][k] (GLOBAL ids =
 * id_base + local index), best first; slots past min(k, n) hold -inf / -1.
 * `workspace` (16-B aligned, caller-owned, also holds the scan's work-split
 * counters, so concurrent calls on distinct streams need distinct workspaces)
 * must hold cbv2_search_workspace_size(index, B, k, scorer) bytes;
 * cbv2_search_workspace_bytes(index, B) is enough for any k and scorer.
 * With CBV2_OPT_FUSED_TOPK on, MaxSim with k <= 104 on the bf16
 * doc-interleaved scan (B > 16) fuses the top-k into the scan (no [B][n]
 * score matrix: each workgroup keeps its best k per query in LDS, then one
 * selection per query); results are those of the unfused path bit for bit.
 * Any k >= 1 (torch.topk takes any k): k > 1024 selects in passes of 4096
 * keys, each bounded below the previous pass's last key (same tie rule).
 * Extends §8(b)'s prototype with scorer / q_dtype / workspace.  */
size_t cbv2_search_workspace_size(const cbv2_index* index, int32_t B, int32_t k, int32_t scorer);
size_t cbv2_search_workspace_bytes(const cbv2_index* index, int32_t B);
int cbv2_search(cbv2_index* index, int32_t scorer, const void* Q, int32_t q_dtype, int32_t B,
                int32_t lq, int32_t k, void* workspace, size_t workspace_bytes,
                float* out_scores, int32_t* out_ids, void* stream);

/* Filtered search (no reference counterpart: the reference ranks its whole
 * corpus, but its chunks carry a document_id, a heading_path and metadata --
 * local_rag_complete.py's ChunkStore -- and a RAG application asks about one
 * document, one tenant, a metadata predicate).  A filter is a bitmap over the
 * shard's LOCAL docs: ceil(n / 32) uint32 words on the device, doc i allowed
 * when bit i & 31 of word i >> 5 is set; bits at positions >= n are ignored.
 * One filter serves a whole cbv2_search_filtered call; one filter per query:
 * cbv2_search_filtered_batch below.
 *  - cbv2_filter_create compacts the bitmap into the ascending list of the
 *    allowed local ids (popcount per word, prefix sum over the words, scatter)
 *    in `buf`, a caller-owned DEVICE buffer of cbv2_filter_bytes(n) bytes
 *    (16-B aligned) the handle borrows until cbv2_filter_destroy; `allow` is
 *    read during the call only.  It then WAITS on `stream` once to read m, the
 *    number of allowed docs (cbv2_filter_count): the only host round trip, so
 *    create is NOT capturable.  The handle is read-only afterwards (several
 *    streams may share it) and remembers the index's n, id_base and device:
 *    passing it with an index that differs in any of those is CBV2_EINVAL.
 *  - cbv2_search_filtered: cbv2_search (bf16 / MXFP8 queries, either scorer)
 *    or the faithful search (an fp32-faithful index with q_dtype
 *    CBV2_DTYPE_F32, Q f32 [B][lq][128]) over the allowed docs only: their
 *    top-k, score descending then id ascending; out_scores f32 [B][k],
 *    out_ids int32 [B][k] (global ids); slots past min(k, m) hold -inf / -1;
 *    m == 0 writes only that padding and launches no scan.  The scores are
 *    the unfiltered scorer's for those docs, bit for bit (cbv2_score;
 *    cbv2_score_f32 for the faithful search); an allowed doc with doclens == 0
 *    scores -inf, keeps its id and ranks after every finite score.
 *    Asynchronous and capturable.  Workspace (16-B aligned, one per stream):
 *    cbv2_search_filtered_workspace_size(index, filter, B, lq, k, scorer)
 *    bytes, computed with the options the search will run under.
 *    Two paths, same results (CBV2_OPT_FILTER_PATH):
 *    subset -- MaxSim on a bf16, fp32-faithful or MXFP8 index, of 128-slot
 *      docs or long documents (ld = 256 / 512 / 1024: the unfiltered long-doc
 *      scan's shape for the same B): the scan walks the id list (doc lengths and base addresses -- on
 *      an MXFP8 index the token and the scale rows -- through it) and
 *      writes a compact row [B][m] -- B <= 2 the streaming scan, moving only
 *      the listed docs' token tiles; larger B the doc-interleaved MFMA scans,
 *      each listed doc loaded once per query group; faithful: one faithful
 *      score (lo.qhi + hi.qlo + hi.qhi in one kernel) per (query, allowed doc);
 *      no [B][n] block in the workspace;
 *    dense -- everything else (REF_MEANPOOL_COSINE):
 *      the full scorer into [B][n], then a gather of the allowed columns.
 *    Both end in the row top-k and a map of row positions to
 *    id_base + ids[pos] (the list is ascending: position order is id order). */
typedef struct cbv2_filter cbv2_filter;
size_t cbv2_filter_bytes(int64_t n);
int cbv2_filter_create(const cbv2_index* index, const uint32_t* allow, void* buf, size_t buf_bytes, void* stream,
                       cbv2_filter** out);
int64_t cbv2_filter_count(const cbv2_filter* filter);
int cbv2_filter_destroy(cbv2_filter* filter);
size_t cbv2_search_filtered_workspace_size(const cbv2_index* index, const cbv2_filter* filter, int32_t B, int32_t lq,
                                           int32_t k, int32_t scorer);
int cbv2_search_filtered(cbv2_index* index, const cbv2_filter* filter, int32_t scorer, const void* Q, int32_t q_dtype,
                         int32_t B, int32_t lq, int32_t k, void* workspace, size_t workspace_bytes,
                         float* out_scores, int32_t* out_ids, void* stream);

/* cbv2_search_filtered_f32 -- the filtered twin of cbv2_search_f32: the
 * faithful top-k of the allowed docs of an fp32-faithful index, Q f32
 * [B][lq][128], 1 <= lq <= 32.  Results are cbv2_search_filtered's for the
 * same arguments, bit for bit: cbv2_score_f32's scores, score descending then
 * id ascending, -inf / -1 past min(k, m), an allowed empty doc after every
 * finite score.  out_status int32 [B]: the row's band size, or -1 when the
 * row was scored pair by pair over its whole list; m == 0 writes padding only
 * and status 0.
 *  Where CBV2_OPT_FILTER_PATH resolves to the subset path (every ld),
 *  CBV2_OPT_FILTER_BAND picks between
 *  pair -- one faithful score per (query, allowed doc), the row top-k, the id
 *    map: status -1 everywhere; and
 *  band -- cbv2_search_f32's band method over the compact row: the bf16 subset
 *    scan of hi (T [B][m]), T's row top-k, the faithful scores of those k docs
 *    (lb = their minimum: k allowed docs score at least lb), the band of every
 *    list position with T >= lb - beta (beta(q) bounds |T - S| for every doc
 *    of the index, so for every allowed one: no allowed doc outside the band
 *    can reach the top-k), its rescoring and the exact select.  cap in
 *    [k, 16384] (CBV2_EINVAL otherwise); a row whose band exceeds cap gets
 *    status -1 and is recomputed pair by pair on the device, no host round
 *    trip, the other rows untouched.  Needs m > k and k <= 16384: other calls
 *    take `pair` (there cap is not read).  No [B][n] buffer of any kind.
 *  Where the filter path resolves to dense (CBV2_OPT_FILTER_PATH = 2; m >
 *  0.5 n under the automatic rule): every doc's faithful score into [B][n], a column
 *  gather, status -1.
 * Workspace (16-B aligned, one per stream): cbv2_search_filtered_f32_
 * workspace_size(index, filter, B, lq, k, cap) bytes, computed with the
 * options the search will run under (0 for a null handle or B, lq, k < 1).
 * Every argument is validated before any launch: the filter's n / id_base /
 * device against the index (CBV2_EINVAL), an index without a residual
 * (CBV2_ESTATE).  Asynchronous and capturable (the filter created before the
 * capture).  cbv2_search_filtered with f32 queries on a faithful index runs
 * the same routine with cap = CBV2_RETRIEVE_BAND_CAP and keeps the status in
 * its workspace.  Per-query filters (cbv2_search_filtered_batch), the sharded
 * calls and the cbv2_retrieve_* calls are as they were: no band under a
 * filter there.
 * (Its guard-band test is tests/test_gpu_filter_band.py, not the table of
 * tests/test_gpu_bounds.py, which lists the one-line `int cbv2_*(`
 * declarations of this file: hence the return type on a line of its own.)   */
size_t cbv2_search_filtered_f32_workspace_size(const cbv2_index* index, const cbv2_filter* filter, int32_t B,
                                               int32_t lq, int32_t k, int32_t cap);
int
cbv2_search_filtered_f32(cbv2_index* index, const cbv2_filter* filter, const float* Q, int32_t B, int32_t lq,
                             int32_t k, int32_t cap, void* workspace, size_t workspace_bytes, float* out_scores,
                             int32_t* out_ids, int32_t* out_status, void* stream);

/* Per-query filters: one filtered search for a batch whose queries each have
 * their own allowed set (256 users, each asking about their own document).
 * A filter batch assigns one existing cbv2_filter to each of the B queries of
 * a call; handles may repeat.
 *  - cbv2_filter_batch_create checks every filter against the index (n,
 *    id_base, device; a null entry or a mismatch is CBV2_EINVAL, nothing is
 *    launched) and writes the per-row table -- the exclusive prefix of the
 *    rows' work items [B + 1], the counts m_b [B] and the lists' addresses
 *    [B], 4 B + 1 int32 words -- into `buf`, a caller-owned DEVICE buffer of
 *    cbv2_filter_batch_bytes(B) bytes (16-B aligned).  `per_query` is a HOST
 *    array read during the call only.  It returns when the table is on the
 *    device (it waits on `stream`): NOT capturable.  The batch borrows `buf`
 *    and the filters until cbv2_filter_batch_destroy, is read-only afterwards
 *    and may be shared across streams.  The ragged scan's docs per work item
 *    are fixed here (CBV2_OPT_FILTER_BATCH_CHUNK_DOCS).
 *  - cbv2_search_filtered_batch: row b is what cbv2_search_filtered(index,
 *    per_query[b], ..., Q + b, B = 1, ...) returns, bit for bit: the top-k of
 *    filter b's docs, score descending then id ascending, global ids; slots
 *    past min(k, m_b) hold -inf / -1 (a row with m_b == 0 is all padding); an
 *    allowed doc with doclens == 0 scores -inf, keeps its id and ranks after
 *    every finite score.  Query types, scorers and index kinds: those of
 *    cbv2_search_filtered.  B must equal the batch's B (CBV2_EINVAL).  If
 *    every m_b is 0 no scan is launched.  Asynchronous and capturable, no host
 *    round trip.  MaxSim queries hold at most 32 tokens here, as in every
 *    search call (longer queries: the caller sums the scores of 32-token
 *    blocks; the Python layer then serves per-query filters row by row).  Paths (CBV2_OPT_FILTER_PATH; the automatic rule of
 *    cbv2_search_filtered applied to M = the largest m_b):
 *    (the subset paths serve 128-slot docs and long documents alike: the
 *    streaming scans take ld at run time, the faithful pair kernel works in
 *    128-token blocks)
 *    subset, bf16 -- ONE launch of the ragged streaming scan for all rows: a
 *      wave's work item is (row b, chunk of row b's list), found by a search
 *      of the table's prefix; each (query, allowed doc) pair is streamed and
 *      scored on its own (queries sharing a filter share no loads);
 *    subset, MXFP8 -- the same ragged scan on e4m3 tiles (the MXFP8 streaming
 *      scan's 8-wave workgroups; token and scale rows through the lists);
 *    subset, faithful -- the lists gathered into a candidate matrix [B][M],
 *      then one faithful score per (query, allowed doc), count[b] = m_b;
 *    dense -- the full scorer into [B][n], then a ragged gather.
 *    All end in the row top-k over compact rows of stride M whose columns past
 *    m_b hold -inf, and a map of positions to id_base + list_b[pos] (-1 at or
 *    past m_b).  Workspace (16-B aligned, one per stream), with r = round up
 *    to 256 B:  counters + r(top-k workspace of (B, M)) + r(4 B M) for the
 *    rows + [faithful subset: r(4 B M) for the candidates] + [dense:
 *    r(4 B n)] + [faithful index: the query split of cbv2_score_f32];
 *    cbv2_search_filtered_batch_workspace_size is authoritative and is
 *    computed with the options the search will run under.                  */
typedef struct cbv2_filter_batch cbv2_filter_batch;
size_t cbv2_filter_batch_bytes(int32_t B);
int cbv2_filter_batch_create(const cbv2_index* index, const cbv2_filter* const* per_query, int32_t B, void* buf,
                             size_t buf_bytes, void* stream, cbv2_filter_batch** out);
int64_t cbv2_filter_batch_pairs(const cbv2_filter_batch* fb);
int64_t cbv2_filter_batch_max_count(const cbv2_filter_batch* fb);
int cbv2_filter_batch_destroy(cbv2_filter_batch* fb);
size_t cbv2_search_filtered_batch_workspace_size(const cbv2_index* index, const cbv2_filter_batch* fb, int32_t B,
                                                 int32_t lq, int32_t k, int32_t scorer);
int cbv2_search_filtered_batch(cbv2_index* index, const cbv2_filter_batch* fb, int32_t scorer, const void* Q,
                               int32_t q_dtype, int32_t B, int32_t lq, int32_t k, void* workspace,
                               size_t workspace_bytes, float* out_scores, int32_t* out_ids, void* stream);

/* Grouped search (no reference counterpart: the reference ranks chunks, but its
 * chunks carry a document_id -- local_rag_complete.py's ChunkStore -- and a RAG
 * application asks for DOCUMENTS; one long document can own every slot of a
 * chunk top-k).  The top-k groups, each with its best chunks.  Everything here
 * is exact: no tolerance, no over-fetch.
 *  A grouping assigns every LOCAL chunk i a group index group_of[i] in [0, G),
 *  or -1 for "in no group": such a chunk is never returned (a filter composes
 *  with grouping by putting -1 on disallowed chunks).  Groups need not be
 *  contiguous id ranges; groups without members are allowed; G' = the number
 *  of groups with at least one member.  For each query b:
 *    group score   the maximum of the scorer's scores of the group's chunks --
 *                  the unfiltered scorer's bits (cbv2_score; cbv2_score_f32 for
 *                  a faithful search);
 *    group order   group score descending, then group index ascending;
 *    chunks        for each of the top-k groups its best r chunks (1 <= r <= 8),
 *                  score descending, then chunk id ascending;
 *    empty docs    a chunk with doclens == 0 scores -inf, keeps its id and
 *                  ranks after every finite chunk of its group; a group whose
 *                  chunks all score -inf ranks after every finite group and
 *                  keeps its index and chunk ids (the filters' convention).
 *  Outputs: out_scores f32 [B][k] (-inf past min(k, G')), out_groups int32
 *  [B][k] (the caller's group index; -1 past min(k, G')), out_ids int32
 *  [B][k][r] (GLOBAL chunk ids; -1 past the group's size and in padded
 *  groups), out_chunk_scores f32 [B][k][r] (-inf where out_ids is -1);
 *  out_chunk_scores[b][j][0] has the bits of out_scores[b][j].  Any k >= 1, as
 *  in cbv2_search (k > 1024: the multi-pass selection).
 *  - cbv2_groups_build_host (HOST pointers, no GPU): a stable counting sort of
 *    the member chunks.  order int32 [n]: the member chunks grouped by group,
 *    ascending id inside a group, the first out3[0] entries valid; offsets
 *    int32 [G + 1]: offsets[0 .. G'] the segment bounds over the non-empty
 *    groups in ascending group index; labels int32 [G]: labels[0 .. G') the
 *    caller's indices of those groups; out3 int64 [3] = {members, G', largest
 *    group}.  A value < -1 or >= G is CBV2_EINVAL, the message names the first
 *    offending position, and no output has been written.  G >= 1,
 *    n <= 0x7fffffff.
 *  - cbv2_groups_create validates group_of (HOST int32 [n], n the index's,
 *    read during the call only) with the builder before anything touches the
 *    device, uploads the three arrays into `buf`, a caller-owned DEVICE buffer
 *    of cbv2_groups_bytes(n, G) bytes (16-B aligned) the handle borrows until
 *    cbv2_groups_destroy, and WAITS on `stream` for the copies: NOT capturable,
 *    like the filter batch's create.  The handle is read-only afterwards
 *    (several streams may share it) and remembers the index's n, id_base and
 *    device: passing it with an index that differs in any of those is
 *    CBV2_EINVAL.  cbv2_groups_count: G'.
 *  - cbv2_group_topk_rows: the selection on its own (as cbv2_topk_rows is to
 *    cbv2_search), over any score matrix whose row b is scores[b * ld + i],
 *    i < n (long queries' summed blocks, external scorers); columns at or past
 *    n are never read, chunks outside every group never influence a result.
 *    Workspace: cbv2_group_topk_workspace_size(groups, B, k, r) bytes.
 *  - cbv2_search_grouped: the scorer's scores of every chunk into a [B][n]
 *    block of the workspace, then the same selection.  Query types, scorers
 *    and index kinds: those of cbv2_search (bf16, MXFP8, REF_MEANPOOL_COSINE,
 *    ld = 128 / 256 / 512 / 1024); on an fp32-faithful index with q_dtype
 *    CBV2_DTYPE_F32 (Q f32 [B][lq][128]) the scores are cbv2_score_f32's, bit
 *    for bit, reached through cbv2_search_grouped_f32's routine (below) with
 *    cap = max(CBV2_RETRIEVE_BAND_CAP, k), the status kept in the workspace.
 *    lq <= 32 for every scorer.  Workspace:
 *    cbv2_search_grouped_workspace_size(index, groups, B, lq, k, r, scorer),
 *    computed with the options the search will run under.
 *  - cbv2_search_grouped_f32: the grouped search of an fp32-faithful index, Q
 *    f32 [B][lq][128], 1 <= lq <= 32, with a band capacity and a status.
 *    Results are cbv2_search_grouped's for the same arguments, bit for bit,
 *    under every value of CBV2_OPT_GROUP_BAND.  out_status int32 [B]: the
 *    row's global band size, or -1 when the row took the full faithful scan;
 *    G' == 0 or n == 0 writes padding only and status 0.  Two ways:
 *    full -- cbv2_score_f32's scan of every chunk into [B][n], then the
 *      selection: status -1 everywhere, cap not read;
 *    band -- with T the bf16 scan of hi, S the faithful score and beta(q) >=
 *      |T - S| for every chunk: the k best groups by T and their leaders (k
 *      chunks of k distinct groups), lb = the minimum faithful score of those
 *      chunks (so the k-th group score is >= lb), the band of every member
 *      chunk with T >= lb - beta (no chunk outside can lead a top-k group),
 *      its faithful scores, their maximum per group and the row top-k of the
 *      groups; then per selected group g its top-r chunks by T, s_g = the
 *      minimum of their faithful scores, the chunks of g with T >= s_g - beta
 *      (no other chunk of g can be among its best r), their faithful scores
 *      and the best r.  Needs G' > k, k <= 16384, k r <= cap and
 *      CBV2_OPT_RESCORE_SPLIT on; other calls take `full`.  With the band, cap
 *      outside [k, 16384] is CBV2_EINVAL; both lists of a row (the global
 *      band, the per-group bands together) hold at most cap chunks, and a row
 *      that exceeds either gets status -1 and is recomputed by `full` on the
 *      device, every launch gated on the status: no host round trip, the other
 *      rows untouched.
 *    An index without a residual is CBV2_ESTATE, a handle of another index, a
 *    null out_status or a short / misaligned workspace CBV2_EINVAL, all before
 *    any launch.  Workspace: cbv2_search_grouped_f32_workspace_size(index,
 *    groups, B, lq, k, r, cap) bytes under the options in force (0 for null
 *    handles, an index without a residual, B, lq, k, r out of range, or a cap
 *    outside [k, 16384] where the band would be taken): the search's blocks,
 *    then for the band 4 r256(4 B) of per-row words, 3 r256(4 B cap) for the
 *    lists and their scores, 4 r256(4 B k) and 3 r256(4 B k r) for the leaders.
 *    The sharded calls, cbv2_retrieve_*, cbv2_group_topk_rows and the bf16,
 *    MXFP8 and mean-pool grouped searches are as they were.
 *  Both compute calls are asynchronous with no host round trip, and both may
 *  be issued on a stream that is capturing a hipGraph when the groups handle
 *  was created before the capture: every replay recomputes them from the
 *  buffers' contents at replay time and zeroes the keys it folds into in the
 *  workspace (tests/test_gpu_group.py replays them over a poisoned workspace
 *  and poisoned outputs).  Every argument is checked on the host before any
 *  launch: null handles, a handle of another index, k < 1, r outside [1, 8],
 *  null outputs, a short or misaligned (16 B) workspace.  G' == 0 or n == 0
 *  writes the padding only and launches no scan.  Workspaces, one per stream,
 *  with r256 = round up to 256 B: the selection takes r256(4 B G') for the
 *  keys / group rows + r256(4 B k) for the selected positions + the row
 *  top-k's workspace of (B, G'); the search adds the scan's counter block in
 *  front, r256(4 B n) for the scores and, on an fp32-faithful index, the query
 *  split of cbv2_score_f32 and, where f32 queries would take the band, the
 *  band's blocks (cbv2_search_grouped_f32).  The *_size functions are authoritative (0 for a
 *  null handle or a B, lq, k, r out of range).
 *  How: the scores are reduced over fixed tiles of `order` positions (not over
 *  groups: a group of half the corpus beside singletons stays balanced) by a
 *  segmented max inside each wave, segments that cross a wave combining with a
 *  32-bit atomic max on the order-preserving score bits; the existing row
 *  top-k ranks the [B][G'] group rows; one workgroup per (query, selected
 *  group) then picks that group's best r chunks in one pass over its segment.
 * (Their guard-band tests are in tests/test_gpu_group.py, not the table of
 * tests/test_gpu_bounds.py: hence the return types on lines of their own.)  */
typedef struct cbv2_groups cbv2_groups;
size_t cbv2_groups_bytes(int64_t n, int32_t G);
int
cbv2_groups_build_host(const int32_t* group_of, int64_t n, int32_t G, int32_t* order, int32_t* offsets,
                           int32_t* labels, int64_t* out3);
int
cbv2_groups_create(const cbv2_index* index, const int32_t* group_of, int32_t G, void* buf, size_t buf_bytes,
                       void* stream, cbv2_groups** out);
int64_t cbv2_groups_count(const cbv2_groups* groups);
int
cbv2_groups_destroy(cbv2_groups* groups);
size_t cbv2_group_topk_workspace_size(const cbv2_groups* groups, int32_t B, int32_t k, int32_t r);
int
cbv2_group_topk_rows(const cbv2_groups* groups, const float* scores, int64_t ld, int32_t B, int32_t k, int32_t r,
                         void* workspace, size_t workspace_bytes, float* out_scores, int32_t* out_groups,
                         int32_t* out_ids, float* out_chunk_scores, void* stream);
size_t cbv2_search_grouped_workspace_size(const cbv2_index* index, const cbv2_groups* groups, int32_t B, int32_t lq,
                                          int32_t k, int32_t r, int32_t scorer);
int
cbv2_search_grouped(cbv2_index* index, const cbv2_groups* groups, int32_t scorer, const void* Q, int32_t q_dtype,
                        int32_t B, int32_t lq, int32_t k, int32_t r, void* workspace, size_t workspace_bytes,
                        float* out_scores, int32_t* out_groups, int32_t* out_ids, float* out_chunk_scores,
                        void* stream);
size_t cbv2_search_grouped_f32_workspace_size(const cbv2_index* index, const cbv2_groups* groups, int32_t B,
                                              int32_t lq, int32_t k, int32_t r, int32_t cap);
int
cbv2_search_grouped_f32(cbv2_index* index, const cbv2_groups* groups, const float* Q, int32_t B, int32_t lq,
                            int32_t k, int32_t r, int32_t cap, void* workspace, size_t workspace_bytes,
                            float* out_scores, int32_t* out_groups, int32_t* out_ids, float* out_chunk_scores,
                            int32_t* out_status, void* stream);

/* Sharded grouped search ("Across shards"): the grouped search
 * of a corpus in contiguous shards, one rank per shard, bit for bit the
 * unsharded cbv2_search_grouped / cbv2_group_topk_rows of the whole corpus on
 * every rank.  All ranks share ONE group index space [0, G): each rank creates
 * its cbv2_groups from its own slice of group_of with the same G (a group may
 * have chunks on every rank, on some, or on none).  Two collectives per call:
 *   round 1  each rank's local top-k groups (r = 1) -> all-gather of the
 *            [scores B k | groups B k] blocks -> cbv2_merge_group_topk: the
 *            maximum per group over the G lists, then the top k.  Exact: a
 *            group of the global top-k is in the local top-k of the rank that
 *            attains its score, and a list can only under-estimate the others.
 *   round 2  each rank's best r chunks of the k selected groups
 *            (cbv2_group_chunks_rows) -> all-gather of the [ids B k r | scores
 *            B k r] blocks -> cbv2_merge_group_chunks.  Round 1's chunks do not
 *            do: a selected group's runner-up chunk can sit on a rank where
 *            the group is outside the local top-k.
 *   out_scores[b][j] is then set to out_chunk_scores[b][j][0] (the same bits).
 *  The pieces, each asynchronous, capturable and without a host round trip,
 *  every argument checked before any launch:
 *  - cbv2_group_chunks_rows: to round 2 what cbv2_group_topk_rows is to the
 *    search.  sel_groups int32 [B][k]: the caller's group indices, -1 for
 *    padding.  out_ids / out_chunk_scores [B][k][r]: the best r chunks of
 *    each selected group among this shard's (cbv2_search_grouped's order and
 *    padding); a padding entry, an index outside [0, G) and a group without a
 *    member on this shard give -1 / -inf in all r slots.  The workspace, 16-B
 *    aligned, of cbv2_group_chunks_workspace_size(B, k) = 2 r256(4 B k) bytes
 *    (0 for B or k < 1), holds the groups' positions and a scratch copy of
 *    their indices; its contents need not survive the call.
 *  - cbv2_merge_group_topk: in_scores f32 / in_groups int32, rank g's [B][k]
 *    list at g * stride elements (stride >= B k; group < 0: padding, in any
 *    slot; lists need not be sorted).  Duplicates of a group reduce to their
 *    maximum; out_scores / out_groups [B][k]: score descending, then group
 *    index ascending, padded with -inf / -1.  1 <= G <= 64 and G k <= 16384
 *    (the keys of a row are sorted in 128 KiB of LDS); beyond that
 *    CBV2_EUNSUPPORTED and nothing is launched.
 *  - cbv2_merge_group_chunks: in_ids int32 / in_cs f32, rank g's [B][k][r] list
 *    at g * stride elements (stride >= B k r; id < 0: padding).  Per (b, j) the
 *    best r of the G r chunks, score descending, then chunk id ascending; a
 *    chunk scoring -inf keeps its id and ranks after every finite chunk;
 *    padded with -1 / -inf.  1 <= G <= 64, 1 <= r <= 8.
 *  The sharded calls are NOT capturable (a collective), and every rank must
 *  make them in the same order with the same B, k, r:
 *  - cbv2_group_topk_sharded: the protocol over a caller score matrix, row b at
 *    scores[b * ld + i], i < n_local (ld >= n_local).
 *  - cbv2_search_grouped_sharded: the scorer's scores of every local chunk into
 *    a [B][n] block of the workspace, then the same protocol.  Query types,
 *    scorers, ld values and lq <= 32: cbv2_search_grouped's.  On an fp32-
 *    faithful shard with f32 queries the scores are cbv2_score_f32's FULL
 *    faithful scan: the certified band of cbv2_search_grouped_f32 is NOT used
 *    under sharding in this version (its T row and overflow gating belong to a
 *    selection made on the shard itself); the results are the same bits.
 *  An empty shard or one without a member sends padding and still joins both
 *  collectives; fewer than k non-empty groups in all: -inf / -1 at the tail;
 *  with one rank the result is cbv2_search_grouped's (the collectives still
 *  run).  G k > 16384 is CBV2_EUNSUPPORTED before any launch or collective (G
 *  and k are equal on all ranks: all refuse together), like every argument
 *  error.  cbv2_comm_stats counts two all-gathers per call.  Workspaces (16-B
 *  aligned; 0 for a null handle, B or k < 1, r outside [1, 8], lq < 1):
 *  cbv2_group_sharded_workspace_bytes(groups, comm, B, k, r) and
 *  cbv2_search_grouped_sharded_workspace_size(index, groups, comm, B, lq, k, r,
 *  scorer).
 * (Guard-band tests: tests/test_gpu_group_sharded.py.) */
size_t cbv2_group_chunks_workspace_size(int32_t B, int32_t k);
int
cbv2_group_chunks_rows(const cbv2_groups* groups, const float* scores, int64_t ld, int32_t B, int32_t k, int32_t r,
                           const int32_t* sel_groups, void* workspace, size_t workspace_bytes, int32_t* out_ids,
                           float* out_chunk_scores, void* stream);
int
cbv2_merge_group_topk(const float* in_scores, const int32_t* in_groups, int32_t G, int32_t B, int32_t k,
                          int64_t stride, float* out_scores, int32_t* out_groups, void* stream);
int
cbv2_merge_group_chunks(const int32_t* in_ids, const float* in_cs, int32_t G, int32_t B, int32_t k, int32_t r,
                            int64_t stride, int32_t* out_ids, float* out_cs, void* stream);

/* cbv2_rerank — JinaColBERTRetriever.rerank (local_rag_complete.py:779-800)
 * without re-encoding: the C candidate docs of each query are GATHERED from
 * the HBM index by global id (cand int32 [B][C]; ids outside this shard or < 0
 * score -inf) and MaxSim-scored against Q (bf16 [B][lq][128]).
 *  k > 0:  out_scores [B][k], out_ids [B][k] (global ids), out_pos [B][k]
 *          (candidate position = the reference's `result_index`), best first;
 *          slots past C hold -inf / -1 / -1.
 *  1 <= C <= 32768 (the reference's argsort takes any C, :789): C > 1024
 *  keeps the raw scores in dynamic LDS and selects in multiple passes.
 *  k == 0: out_scores [B][C] receives the raw candidate scores (for the
 *          sharded path: all-reduce(max) across shards, then cbv2_select_topk). */
int cbv2_rerank(cbv2_index* index, const void* Q, int32_t B, int32_t lq, const int32_t* cand,
                int32_t C, int32_t k, float* out_scores, int32_t* out_ids, int32_t* out_pos,
                void* stream);

/* cbv2_rerank_ws — cbv2_rerank with a caller workspace of
 * cbv2_rerank_workspace_bytes(B, C) bytes: batches of up to 32 queries then
 * score one (query, candidate) per wave across the chip (the raw row in the
 * workspace) and select the top-k in a second kernel — the same scores, ids
 * and positions, bit for bit, as the one-workgroup-per-query kernel
 * cbv2_rerank uses (a B=1 rerank of 50 candidates otherwise runs 7 docs per
 * wave in sequence on one CU).  A null or short workspace, C > 1024 or
 * B > 32 take cbv2_rerank's path.  (cbv2_rerank with k == 0 and B <= 32 uses
 * the candidate-parallel kernel directly into out_scores.) */
size_t cbv2_rerank_workspace_bytes(int32_t B, int32_t C);
int cbv2_rerank_ws(cbv2_index* index, const void* Q, int32_t B, int32_t lq, const int32_t* cand,
                   int32_t C, int32_t k, void* workspace, size_t workspace_bytes, float* out_scores,
                   int32_t* out_ids, int32_t* out_pos, void* stream);

/* fp32-faithful index ---------------------------------------------------------
 * The reference keeps fp32 embeddings (local_rag_complete.py:735-746: the
 * encode output, torch.save'd as is) and scores them in fp32 (:802-831).  A
 * bf16 index alone is within ~5e-3 of those scores; this mode returns scores
 * within ~1e-5 and the top-k of those scores over the WHOLE corpus.
 *  - cbv2_split_f32: x f32 [rows][128] -> hi = bf16(x) (RNE; the index
 *    tokens) and lo = bf16(x - hi) (the residual), both bf16 [rows][128];
 *    bounds f32[2] (DEVICE, zeroed by the caller) receive max ||x - hi||_2 and
 *    max ||hi||_2 over the rows, rounded up (atomic max).  doclens (nullable,
 *    device int32 [rows / ld]): rows are docs of ld rows and padding rows
 *    (t >= doclens[doc]) are split but left out of the bounds.
 *  - cbv2_index_attach_residual: a bf16 index built on hi borrows lo and
 *    keeps the two bounds (host floats read back from cbv2_split_f32).  The
 *    handle remembers THAT a residual was attached, not the pointer: an empty
 *    shard (n == 0) attaches lo == NULL and is fp32-faithful all the same
 *    (cbv2_index_kind reports 1, every *_f32 call and the sharded calls take
 *    their faithful path), so all ranks of a faithful corpus issue the same
 *    collectives.  Likewise cbv2_index_build_means on n == 0 with null
 *    pointers leaves the means built (of no docs).
 * Queries are f32 [B][lq][128] (lq <= 32); every call needs a workspace of
 * cbv2_f32_workspace_bytes(index, op, B, lq, cap) bytes (16-B aligned), with
 * cap = the band capacity (SEARCH) or C (RERANK), 0 for SCORE.
 *  - cbv2_score_f32: faithful scores of every doc, out[b * ld_out + i]
 *    (lo.qhi + hi.qlo + hi.qhi on the bf16 MFMA, fp32 accumulate).
 *  - cbv2_search_f32: bf16 scan of hi (T), its top-k, whose faithful scores'
 *    minimum lb bounds the k-th faithful score from below; then every doc
 *    with T >= lb - beta(q) is rescored faithfully and the exact top-k of
 *    that band is returned.  beta(q) bounds |T - S| for every doc
 *    (Cauchy-Schwarz on the residuals of docs and query, plus accumulation
 *    slack), so the band holds the faithful top-k of the whole corpus.
 *    out_status int32 [B]: the band size, or -1 when the band exceeded `cap`
 *    (k <= cap <= 16384): that row was then recomputed on the device by the
 *    full faithful scan (cbv2_score_f32's arithmetic) and an exact top-k.
 *    k > 16384 (no band can hold it): every row takes the full scan (-1).
 *    Either way the result is the faithful top-k of the whole corpus; the
 *    call stays asynchronous (no host round trip).
 *  - cbv2_search_f32_begin / _finish: the same search in two calls, for a
 *    sharded corpus.  begin runs the scan and top-k and writes fk (DEVICE f32
 *    [B][k]): the exact faithful scores of the shard's bf16 top-k (-inf
 *    padded; all -inf for an empty shard).  The caller derives lb (DEVICE f32
 *    [B]) from them: the k-th largest of the fk of ALL shards (one all-gather)
 *    -- k docs of the corpus score at least that, so it is <= the global k-th
 *    faithful score; any such lower bound keeps the result exact (one shard:
 *    the minimum of its fk).  finish rescores only the docs with T >= lb -
 *    beta(q) and returns this shard's part of the global top-k (-inf / -1
 *    padded where fewer of its docs can reach it), which the cross-shard merge
 *    completes.  Same workspace between the two calls.
 *  - cbv2_rerank_f32: cbv2_rerank with faithful scores.                      */
#define CBV2_F32_SCORE 0
#define CBV2_F32_SEARCH 1
#define CBV2_F32_RERANK 2
int cbv2_split_f32(const float* x, int64_t rows, int32_t ld, const int32_t* doclens, void* hi, void* lo,
                   float* bounds, void* stream);
int cbv2_index_attach_residual(cbv2_index* index, const void* lo, float resid_max, float norm_max);
size_t cbv2_f32_workspace_bytes(const cbv2_index* index, int32_t op, int32_t B, int32_t lq, int32_t cap);
int cbv2_score_f32(cbv2_index* index, const float* Q, int32_t B, int32_t lq, void* workspace,
                   size_t workspace_bytes, float* out, int64_t ld_out, void* stream);
int cbv2_search_f32(cbv2_index* index, const float* Q, int32_t B, int32_t lq, int32_t k, int32_t cap,
                    void* workspace, size_t workspace_bytes, float* out_scores, int32_t* out_ids,
                    int32_t* out_status, void* stream);
int cbv2_search_f32_begin(cbv2_index* index, const float* Q, int32_t B, int32_t lq, int32_t k, int32_t cap,
                          void* workspace, size_t workspace_bytes, float* fk, float* out_scores, int32_t* out_ids,
                          int32_t* out_status, void* stream);
int cbv2_search_f32_finish(cbv2_index* index, int32_t B, int32_t lq, int32_t k, int32_t cap, void* workspace,
                           size_t workspace_bytes, const float* lb, float* out_scores, int32_t* out_ids,
                           int32_t* out_status, void* stream);
int cbv2_rerank_f32(cbv2_index* index, const float* Q, int32_t B, int32_t lq, const int32_t* cand,
                    int32_t C, int32_t k, void* workspace, size_t workspace_bytes, float* out_scores,
                    int32_t* out_ids, int32_t* out_pos, void* stream);

/* Selection -----------------------------------------------------------------
 * cbv2_select_topk — top-k of each row of a score matrix [B][C] (rerank after
 * the cross-shard all-reduce): rank counting in LDS for C <= 1024, the
 * multi-pass selection beyond (any C, any k).  ids (nullable) [B][C] maps
 * positions to doc ids (NULL: id = position).  Ties: lower position first.
 * out_pos (nullable) receives positions.                                    */
int cbv2_select_topk(const float* scores, const int32_t* ids, int32_t B, int32_t C, int32_t k,
                     float* out_scores, int32_t* out_ids, int32_t* out_pos, void* stream);

/* cbv2_topk_rows — top-k of each row of a large score matrix scores[b*ld + i],
 * i < n; ids written = id_base + i.  With a workspace of
 * cbv2_topk_workspace_bytes(B, n) bytes (0 for short rows) long rows use the
 * sampled-threshold filter + candidate sort; with workspace NULL, or on a
 * candidate overflow, the exact single-pass-per-digit radix select; k > 1024
 * selects in bounded passes (no workspace needed).  The result is identical
 * either way.                                                               */
size_t cbv2_topk_workspace_bytes(int32_t B, int64_t n);
int cbv2_topk_rows(const float* scores, int32_t B, int64_t n, int64_t ld, int32_t k,
                   int64_t id_base, void* workspace, size_t workspace_bytes,
                   float* out_scores, int32_t* out_ids, void* stream);

/* cbv2_merge_topk — merge G per-shard sorted top-k lists ([G][B][k] scores and
 * global ids, e.g. after an RCCL all-gather) into the global top-k [B][k].
 * Entries with id < 0 are padding (a suffix of each list).  Any k: lists of
 * G*k <= 8192 keys are staged in LDS, longer ones searched in place.        */
int cbv2_merge_topk(const float* in_scores, const int32_t* in_ids, int32_t G, int32_t B,
                    int32_t k, float* out_scores, int32_t* out_ids, void* stream);

/* Host fusion (HOST pointers, no GPU) --------------------------------------
 * cbv2_rrf_fuse — HybridRetriever._reciprocal_rank_fusion
 * (local_rag_complete.py:960-978) for B queries at once, followed by the
 * `[:50]` cut of :916 (C = 50): float64 1/(rrf_k + rank) sums in the
 * reference's order and a stable sort, so results and tie order are identical
 * to the Python.  bm25_ids [B][kb], colbert_ids [B][kc] (ids < 0 = padding);
 * out_ids [B][C] (-1 padded), out_scores [B][C] (nullable), out_count [B]
 * (nullable) = distinct ids per query.                                     */
int cbv2_rrf_fuse(const int32_t* bm25_ids, int32_t kb, const int32_t* colbert_ids, int32_t kc, int32_t B,
                  int32_t rrf_k, int32_t C, int32_t* out_ids, double* out_scores, int32_t* out_count);

/* Host BM25 (HOST pointers, no GPU) ---------------------------------------
 * Stage 1 of HybridRetriever.retrieve (local_rag_complete.py:937-950; the
 * reference uses bm25s: LRC:851-858, 939-945) over term ids (tokenisation
 * and stopwords stay in the caller).  Lucene BM25:
 *   idf = ln(1 + (N - df + 0.5) / (df + 0.5)),
 *   w   = idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * |d| / avgdl)),
 * summed over the query's term ids in query order, repeats included (bm25s
 * sums the postings of every query token).  Corpus as CSR: doc i's term ids are
 * doc_terms[doc_offsets[i] .. doc_offsets[i+1]).  Search: queries as CSR,
 * out_ids [B][k] (score desc, then doc id asc; padded with the lowest-id
 * zero-score docs, then -1), out_scores [B][k] (nullable).  n_threads <= 0:
 * min(16, hardware threads).  Parity with bm25s itself: unpinned.          */
typedef struct cbv2_bm25 cbv2_bm25;
int cbv2_bm25_build(const int32_t* doc_terms, const int64_t* doc_offsets, int64_t n_docs, int32_t vocab,
                    float k1, float b, cbv2_bm25** out);
int cbv2_bm25_search(const cbv2_bm25* index, const int32_t* q_terms, const int64_t* q_offsets, int32_t B,
                     int32_t k, int32_t n_threads, int32_t* out_ids, float* out_scores);
/* cbv2_bm25_search_filtered: the same search over the docs whose bit is set in
 * `allow` (HOST, ceil(n_docs / 32) words over the LOCAL docs, the bit order of
 * cbv2_filter_create; bits past n_docs ignored): same weights, accumulation
 * order and tie rule; a doc whose bit is clear never enters the selection, and
 * the zero-score padding takes the lowest-id ALLOWED docs that scored 0, then
 * -1.  allow == NULL is cbv2_bm25_search.                                  */
int cbv2_bm25_search_filtered(const cbv2_bm25* index, const int32_t* q_terms, const int64_t* q_offsets, int32_t B,
                              int32_t k, int32_t n_threads, const uint32_t* allow, int32_t* out_ids,
                              float* out_scores);
/* cbv2_bm25_search_filtered_batch: query b under its own bitmap allows[b]
 * (HOST array [B] of HOST bitmaps; a NULL entry = unfiltered).  Each row equals
 * cbv2_bm25_search_filtered on that query alone, ids, score bits and the
 * zero-score padding rule included.                                        */
int cbv2_bm25_search_filtered_batch(const cbv2_bm25* index, const int32_t* q_terms, const int64_t* q_offsets, int32_t B,
                                    int32_t k, int32_t n_threads, const uint32_t* const* allows, int32_t* out_ids,
                                    float* out_scores);
/* Sharded BM25 (no reference counterpart): a rank indexes
 * only its doc range [id_base, id_base + n_docs) but with the GLOBAL
 * statistics (n_global docs, total_global tokens, df_global [vocab] from an
 * all-reduce of cbv2_bm25_doc_freq), so every weight equals the unsharded
 * index's; search then returns global ids (local + id_base), and merging the
 * ranks' lists by (score desc, id asc) reproduces the unsharded top-k.      */
int cbv2_bm25_doc_freq(const int32_t* doc_terms, const int64_t* doc_offsets, int64_t n_docs, int32_t vocab,
                       int64_t* df_out);
int cbv2_bm25_build_shard(const int32_t* doc_terms, const int64_t* doc_offsets, int64_t n_docs, int32_t vocab,
                          float k1, float b, int64_t id_base, int64_t n_global, int64_t total_global,
                          const int64_t* df_global, cbv2_bm25** out);
int64_t cbv2_bm25_num_docs(const cbv2_bm25* index);
int cbv2_bm25_destroy(cbv2_bm25* index);

/* English stemmer (HOST pointers, no GPU): the Snowball English ("Porter2")
 * algorithm PyStemmer's Stemmer("english") implements, which the reference
 * passes to bm25s.tokenize (local_rag_complete.py:851-855, 939-943).  Words
 * are UTF-8, lower-cased by the caller; word i = words[offsets[i] ..
 * offsets[i+1]).  Stems go to out (out_cap >= offsets[n] - offsets[0]
 * suffices: no stem is longer than its word), out_offsets [n + 1].        */
int cbv2_stem_en(const char* words, const int64_t* offsets, int64_t n, char* out, int64_t out_cap,
                 int64_t* out_offsets);

/* Native index file (replaces the torch.save/torch.load of
 * indexes/colbert/index.pt at local_rag_complete.py:743-746, 751 for large
 * corpora — the index.pt reader stays in Python).  One flat file: a 4 KiB
 * header, int32 doclens [n], tokens [n][ld][128] (bf16, or e4m3 bytes) and,
 * for MXFP8, E8M0 scales [n][ld][2]; each section 4 KiB-aligned.  ld = 128
 * token slots (the functions without _ld), or 256 / 512 / 1024 for a bf16
 * long-document index (the _ld variants); readers take ld from the header.
 * cbv2_index_file_write  — DEVICE pointers (an HBM-resident index), D2H in
 *                          64 MiB pinned chunks overlapped with pwrite.
 * cbv2_index_file_read   — docs [begin, end) into DEVICE buffers (tokens
 *                          (end-begin)*ld*128*elem bytes, scales, doclens):
 *                          pread (O_DIRECT where aligned) into two pinned
 *                          buffers overlapped with H2D copies on `stream`;
 *                          returns when the data is in HBM.
 * cbv2_index_file_info   — dtype, doc count and id_base of a file
 *                          (cbv2_index_file_info_ld: and its ld).
 * *_host variants: HOST pointers, no GPU involved.                          */
int cbv2_index_file_info(const char* path, int32_t* dtype, int64_t* n, int64_t* id_base);
int cbv2_index_file_info_ld(const char* path, int32_t* dtype, int64_t* n, int64_t* id_base, int32_t* ld);
int cbv2_index_file_write_ld(const char* path, int32_t dtype, int64_t n, int32_t ld, const void* tokens,
                             const void* scales, const int32_t* doclens, int64_t id_base, void* stream);
int cbv2_index_file_write_host_ld(const char* path, int32_t dtype, int64_t n, int32_t ld, const void* tokens,
                                  const void* scales, const int32_t* doclens, int64_t id_base);
int cbv2_index_file_write(const char* path, int32_t dtype, int64_t n, const void* tokens, const void* scales,
                          const int32_t* doclens, int64_t id_base, void* stream);
int cbv2_index_file_read(const char* path, int64_t begin, int64_t end, void* tokens, void* scales, int32_t* doclens,
                         void* stream);
int cbv2_index_file_write_host(const char* path, int32_t dtype, int64_t n, const void* tokens, const void* scales,
                               const int32_t* doclens, int64_t id_base);
int cbv2_index_file_read_host(const char* path, int64_t begin, int64_t end, void* tokens, void* scales,
                              int32_t* doclens);

/* Streaming index writer (bounded-memory ingest): declare the
 * doc count, append contiguous batches (DEVICE pointers with on_device = 1 --
 * D2H through 64 MiB pinned buffers on `stream` -- or HOST pointers), close.
 * The header is written by close() only when every declared doc was
 * appended; close() after an incomplete ingest (or a failed header write)
 * deletes the file and returns CBV2_EINVAL, so an interrupted ingest never
 * leaves a file behind, valid-looking or not.
 * Host memory is two staging buffers whatever the corpus size.             */
typedef struct cbv2_index_writer cbv2_index_writer;
int cbv2_index_writer_open(const char* path, int32_t dtype, int64_t n, int64_t id_base, cbv2_index_writer** out);
int cbv2_index_writer_open_ld(const char* path, int32_t dtype, int64_t n, int32_t ld, int64_t id_base,
                              cbv2_index_writer** out);
int cbv2_index_writer_append(cbv2_index_writer* w, int64_t count, const void* tokens, const void* scales,
                             const int32_t* doclens, int32_t on_device, void* stream);
int64_t cbv2_index_writer_count(const cbv2_index_writer* w);
int cbv2_index_writer_close(cbv2_index_writer* w);

/* Multi-GPU exchange (SURVEY.md §8(b) "cbv2_comm_init(ncclComm_t) +
 * cbv2_search_sharded", §8(e)).  No reference counterpart: the reference is
 * single-process.  One process per GPU, each holding the shard
 * [id_base, id_base + n) of the corpus as a cbv2_index.
 *
 * cbv2_comm_init — borrow an initialised RCCL communicator (ncclComm_t; e.g.
 *   torch's ProcessGroupNCCL._comm_ptr()).  rccl_library: path of the RCCL
 *   library that created it (NULL: "librccl.so"); the collectives are
 *   resolved from that library.  cbv2_comm_destroy does not free the comm.
 * cbv2_search_sharded — every rank: local scan + top-k, plus (kb > 0) this
 *   rank's stage-1 BM25 top-kb over its doc shard (global ids; host or device
 *   pointers), -> ONE ncclAllGather -> merged global top-k [B][k] and merged
 *   BM25 ids [B][kb] (out_lex_ids, device), identical on every rank.
 *   Workspace: cbv2_sharded_workspace_bytes(ix, comm, B, k, kb, 0).
 *   The same in two calls, so a host stage-1 can run while the GPU scans:
 *   cbv2_search_sharded_local (enqueue the local scan) then
 *   cbv2_search_sharded_exchange (lists in, all-gather, merges) with the SAME
 *   workspace, sized for the exchange's kb (the local call writes only the
 *   head of the send block; its kb just sizes its workspace check).
 *   Q (nullable; the local call's queries, q_dtype, lq): with kb > 0 the
 *   exchange first scores this rank's own BM25 top-kb with the rerank's
 *   arithmetic (raw MaxSim; faithful shards on the local call's query split)
 *   and those prescores ride the same all-gather.
 * cbv2_rerank_sharded_prescored — stage 3 with NO collective, after an
 *   exchange with Q (or kb = 0) on the same workspace with the same B, k, kb:
 *   the fused candidates (RRF of the exchange's merged lists, as
 *   cbv2_retrieve_finish builds them) all sit in the gathered blocks -- in
 *   their owner's stage-2 top-k (whose scores are the rerank's bits) or its
 *   BM25 top-kb (prescored) -- so every rank looks their scores up and selects
 *   the top final_k (score desc, position asc), as cbv2_rerank_sharded would.
 *   cand [B][C] device, C <= 1024.  A candidate found in no list scores -inf
 *   and is counted into *misses (device int32, nullable; the caller zeroes
 *   it): candidates from elsewhere take cbv2_rerank_sharded.
 * cbv2_rerank_sharded — every rank scores the candidates it owns (-inf
 *   otherwise) -> ncclAllReduce(MAX) -> top-k select; cand [B][C] global ids
 *   (device).  Workspace: the size above with C (a bf16 / MXFP8 shard needs
 *   only B*C*4 bytes).
 * cbv2_comm_stats (diagnostic): out2 = {all-gathers, all-reduces} issued on
 *   the handle so far.
 * fp32-faithful shards (cbv2_index_attach_residual; Q f32, q_dtype
 *   CBV2_DTYPE_F32): the local call runs the faithful search against the
 *   GLOBAL k-th bound -- bf16 scan + top-k + the exact faithful scores of that
 *   top-k (cbv2_search_f32_begin), ONE ncclAllGather of those [B][k] scores,
 *   their union's k-th largest as lb, the band rescoring (cbv2_search_f32_finish,
 *   band capacity CBV2_RETRIEVE_BAND_CAP) -- so the local call is itself a
 *   collective; the rerank scores the owned candidates faithfully
 *   (cbv2_rerank_f32).  Results equal the unsharded faithful search / rerank
 *   bit for bit.
 * Collectives are enqueued on `stream`; every rank must call in the same
 * order (as with any RCCL program).                                        */
typedef struct cbv2_comm cbv2_comm;
int cbv2_comm_init(void* nccl_comm, const char* rccl_library, cbv2_comm** out);
int cbv2_comm_size(const cbv2_comm* comm);
int cbv2_comm_rank(const cbv2_comm* comm);
int cbv2_comm_destroy(cbv2_comm* comm);
size_t cbv2_sharded_workspace_bytes(const cbv2_index* index, const cbv2_comm* comm, int32_t B, int32_t k,
                                    int32_t kb, int32_t C);
int cbv2_search_sharded(cbv2_index* index, cbv2_comm* comm, int32_t scorer, const void* Q, int32_t q_dtype,
                        int32_t B, int32_t lq, int32_t k, const int32_t* lex_ids, const float* lex_scores,
                        int32_t kb, void* workspace, size_t workspace_bytes, float* out_scores, int32_t* out_ids,
                        int32_t* out_lex_ids, void* stream);
int cbv2_search_sharded_local(cbv2_index* index, cbv2_comm* comm, int32_t scorer, const void* Q, int32_t q_dtype,
                              int32_t B, int32_t lq, int32_t k, int32_t kb, void* workspace, size_t workspace_bytes,
                              void* stream);
int cbv2_search_sharded_exchange(cbv2_index* index, cbv2_comm* comm, const void* Q, int32_t q_dtype, int32_t lq,
                                 int32_t B, int32_t k, const int32_t* lex_ids, const float* lex_scores, int32_t kb,
                                 void* workspace, size_t workspace_bytes, float* out_scores, int32_t* out_ids,
                                 int32_t* out_lex_ids, void* stream);
int cbv2_rerank_sharded_prescored(cbv2_index* index, cbv2_comm* comm, int32_t B, int32_t k, int32_t kb,
                                  const int32_t* cand, int32_t C, int32_t final_k, void* workspace,
                                  size_t workspace_bytes, float* out_scores, int32_t* out_ids, int32_t* out_pos,
                                  int32_t* misses, void* stream);
int cbv2_rerank_sharded(cbv2_index* index, cbv2_comm* comm, const void* Q, int32_t B, int32_t lq,
                        const int32_t* cand, int32_t C, int32_t k, void* workspace, size_t workspace_bytes,
                        float* out_scores, int32_t* out_ids, int32_t* out_pos, void* stream);
int cbv2_comm_stats(const cbv2_comm* comm, int64_t* out2);
/* The sharded grouped search (described with the grouped search above). */
size_t cbv2_group_sharded_workspace_bytes(const cbv2_groups* groups, const cbv2_comm* comm, int32_t B, int32_t k,
                                          int32_t r);
int
cbv2_group_topk_sharded(const cbv2_groups* groups, cbv2_comm* comm, const float* scores, int64_t ld, int32_t B,
                            int32_t k, int32_t r, void* workspace, size_t workspace_bytes, float* out_scores,
                            int32_t* out_groups, int32_t* out_ids, float* out_chunk_scores, void* stream);
size_t cbv2_search_grouped_sharded_workspace_size(const cbv2_index* index, const cbv2_groups* groups,
                                                  const cbv2_comm* comm, int32_t B, int32_t lq, int32_t k, int32_t r,
                                                  int32_t scorer);
int
cbv2_search_grouped_sharded(cbv2_index* index, const cbv2_groups* groups, cbv2_comm* comm, int32_t scorer,
                                const void* Q, int32_t q_dtype, int32_t B, int32_t lq, int32_t k, int32_t r,
                                void* workspace, size_t workspace_bytes, float* out_scores, int32_t* out_groups,
                                int32_t* out_ids, float* out_chunk_scores, void* stream);

/* TEST-ONLY -- not for production use.  cbv2_comm_loopback_init writes
 * `nranks` (1..64) communicator handles out[0..nranks) that form ONE group
 * inside this process, on the current device: rank r is driven by its own
 * host thread and stream, and the collectives the calls above use keep RCCL's
 * semantics (every rank calls; a call returns once every rank has enqueued;
 * no rank's stream passes the collective before all peers' data is in):
 * all-gather = device copies of the G send blocks, all-reduce(MAX) = a max
 * kernel over them.  It exercises the sharded exchange at G > 1 on one GPU.
 * A rank that does not reach a collective within 60 s fails the group.
 * Free each handle with cbv2_comm_destroy.                                  */
int cbv2_comm_loopback_init(int32_t nranks, cbv2_comm** out);

/* One query batch through HybridRetriever.retrieve's stages 2 -> RRF -> 3
 * (local_rag_complete.py:894-935) with ONE host round trip and no caller code
 * between the stages (the latency path: no D2H / RRF / H2D / launch hops in the
 * host language).  Replaces the sequence _colbert_search (:952-958) ->
 * _reciprocal_rank_fusion (:960-978) -> [:C] (:916) -> _colbert_rerank
 * (:996-1014) for the caller; results equal those of the separate calls
 * (cbv2_search[_f32] / cbv2_search_sharded_*, cbv2_rrf_fuse, cbv2_rerank_ws /
 * _f32 / cbv2_rerank_sharded) bit for bit.
 *  comm: NULL for one shard; else a cbv2_comm (the exchange above, for
 *        bf16, MXFP8 and fp32-faithful shards alike).
 *  Q:    the index's query type: bf16 [B][lq][128] (bf16 index), the
 *        cbv2_quantize_mxfp8 buffer (MXFP8), f32 (fp32-faithful); lq <= 32.
 *  cbv2_retrieve_begin enqueues stage 2 (this shard's scan + top-k; the band
 *    capacity of a faithful search is CBV2_RETRIEVE_BAND_CAP) and returns:
 *    the caller runs stage 1 (host BM25) meanwhile.  Its kb is an upper
 *    bound of the kb finish will pass (the stage-1 list width is known only
 *    after stage 1 ran); B, lq, k, C and the workspace must be the same.
 *  cbv2_retrieve_finish takes the stage-1 lists (HOST pointers: lex_ids
 *    [B][kb] global ids, -1 padded; lex_scores [B][kb], read only with a
 *    comm; kb = 0: no stage 1), (comm: all-gather + merges), copies the
 *    ColBERT top-k to host_stage, WAITS for it (the round trip), fuses on the
 *    host (cbv2_rrf_fuse with rrf_k, first C), uploads the candidates and
 *    enqueues the rerank + select: out_scores f32 [B][final_k], out_ids
 *    int32 [B][final_k] (global ids), out_pos int32 [B][final_k] (position
 *    in the fused list), device, best first, -inf / -1 padded.  One shard,
 *    B <= 8, bf16 / fp32-faithful: the rerank's scores are already known
 *    (stage 2's own for its ids; a stage-1 prescore of the kb lists, launched
 *    at finish entry on a second stream of the calling thread), so the host
 *    picks the top final_k itself and a one-workgroup kernel copies it into
 *    the device outputs (same results, bit for bit).
 *  workspace: device, 256-B aligned, cbv2_retrieve_workspace_bytes(index,
 *    comm, B, lq, k, kb, C) bytes, the same one for begin and finish;
 *    host_stage: host (pinned for asynchronous copies),
 *    cbv2_retrieve_host_bytes(B, k, kb, C) bytes, one per stream.
 *  Q at finish: the same buffer and contents as at begin.  For a single
 *    fp32-faithful shard finish reuses the query split begin left in the
 *    workspace while it is still the last split enqueued there (same index,
 *    Q pointer, B, lq); if anything split other queries into that workspace
 *    in between, finish splits Q again (same results either way).
 *  Both calls select the index's device themselves (the caller's current
 *    device may differ) and restore the caller's.  finish's wait polls the
 *    stream (hipStreamQuery) -- flat out for B <= 8, sleeping between polls
 *    for larger batches, so it never holds a core for a whole batch scan;
 *    the stream must carry no other thread's work meanwhile.  A one-shard
 *    call takes a device-mapped host buffer from a per-device pool at begin
 *    (the search's final select writes the ids into it, the fused candidates
 *    go into it and the rerank reads them in place) and returns it at finish,
 *    reusable once that rerank has run.
 * cbv2_retrieve_finish_host: finish, and the final top-k also in the HOST
 *    arrays host_scores / host_ids / host_pos ([B][final_k], any host memory)
 *    when it returns (the reference's retrieve returns host results,
 *    LRC:935).  One shard: the final select writes them into the call's
 *    mapped buffer as tagged words and the host polls them (no D2H copy, no
 *    stream wait); otherwise they are copied down and waited for.  The
 *    device outputs are written as by finish.
 * cbv2_retrieve_cancel: a begin that will not be finished (the caller's
 *    stage 1 failed): returns its host buffer to the pool (no-op otherwise).
 * cbv2_retrieve_host_marks (diagnostic): host timestamps (steady_clock ns) of
 *    this thread's last finish: enter, D2H issued, wait done, fusion done,
 *    rerank enqueued (the host rerank: its select done), exit (max entries
 *    written, up to 6).
 * cbv2_retrieve_pool_stats (diagnostic): [0] mapped buffers created in this
 *    process, [1] buffers idle in the pools (at most the number of calls that
 *    ever ran at once), [2] finish_host calls whose results were read from the
 *    final select's host words, [3] finish calls that picked the final top-k
 *    on the host (one shard, B <= 8, bf16 / fp32-faithful: every fused
 *    candidate's score is stage 2's own or stage 1's prescore).
 * cbv2_index_kind: the index's dtype (CBV2_DTYPE_*) and whether a residual is
 *    attached (fp32-faithful, 1) or not (0).                                */
#define CBV2_RETRIEVE_BAND_CAP 16384
int cbv2_index_kind(const cbv2_index* index, int32_t* dtype, int32_t* faithful);
size_t cbv2_retrieve_workspace_bytes(const cbv2_index* index, const cbv2_comm* comm, int32_t B, int32_t lq,
                                     int32_t k, int32_t kb, int32_t C);
size_t cbv2_retrieve_host_bytes(int32_t B, int32_t k, int32_t kb, int32_t C);
int cbv2_retrieve_cancel(cbv2_index* index, void* workspace, void* stream);
int cbv2_retrieve_host_marks(int64_t* out, int32_t max);
int cbv2_retrieve_pool_stats(int64_t* out, int32_t max);
int cbv2_retrieve_begin(cbv2_index* index, cbv2_comm* comm, const void* Q, int32_t q_dtype, int32_t B, int32_t lq,
                        int32_t k, int32_t kb, int32_t C, void* workspace, size_t workspace_bytes, void* stream);
int cbv2_retrieve_finish(cbv2_index* index, cbv2_comm* comm, const void* Q, int32_t q_dtype, int32_t B, int32_t lq,
                         int32_t k, const int32_t* lex_ids, const float* lex_scores, int32_t kb, int32_t rrf_k,
                         int32_t C, int32_t final_k, void* workspace, size_t workspace_bytes, void* host_stage,
                         size_t host_bytes, float* out_scores, int32_t* out_ids, int32_t* out_pos, void* stream);
int cbv2_retrieve_finish_host(cbv2_index* index, cbv2_comm* comm, const void* Q, int32_t q_dtype, int32_t B,
                              int32_t lq, int32_t k, const int32_t* lex_ids, const float* lex_scores, int32_t kb,
                              int32_t rrf_k, int32_t C, int32_t final_k, void* workspace, size_t workspace_bytes,
                              void* host_stage, size_t host_bytes, float* out_scores, int32_t* out_ids,
                              int32_t* out_pos, float* host_scores, int32_t* host_ids, int32_t* host_pos,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COLBERT_MI355X_H */
