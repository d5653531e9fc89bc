/*
 * defuse_ptext.h — C ABI of the MI355X prediction text ("ptext"): splitreads.seq and splitreads.break as finished bytes.
 *
 * Replaces, for all groups of a prediction at once, the two writers that follow SplitAlignmentTask::Evaluate:
 *
 *     WriteSequence    tools/SplitAlignment.cpp:596-605   -> ptext_format, the .seq text
 *     WriteBreak       tools/SplitAlignment.cpp:607-615   -> ptext_format, the .break text
 *
 * It ends the resident chain (cand_enumerate_device, bat_assemble_device, dsa_upload_device / dsa_run,
 * dsa_copy_records_device, rec_*, eval_groups_device, pred_predict_resident): with rec_text for splitreads.alignments and
 * splitreads.predalign, a caller of the chain sends alignments up and gets the bytes of all three files down, and keeps no
 * formatting code and no loop over the groups.
 *
 * Per group g of the latest successful pred_predict* of a pred_ctx, in group order:
 *     .seq    "%d\t" fusion_id, the sequence bytes, "\t0\t", "%lld\t" count, %g(pos_avg), "\t", %g(min_avg), "\n"
 *     .break  for cluster end 0, then 1:  "%d\t%d\t" fusion_id, end, the end's reference name, "\t+\t" or "\t-\t" by the end's
 *             ALIGN strand (mAlignStrand of the regions file; not pred_task.seq_strand), "%d\n" break_pos[end]
 * "%g" is an ostream's default print of a double: precision 6, the text glibc's printf("%g") gives in the C locale.
 *
 * Which groups get which lines:
 *   - EVAL_NO_SPLIT and a task: the tool's lines of a group without a split - sequence "N", count 0, "-1" and "-1", break
 *     positions 0;
 *   - PRED_NO_TASK or PRED_OUT_OF_WINDOW: no line in either text (the reference evaluates a default task or exits there);
 *   - EVAL_HOST_STATS (with a split), or an average the formatter does not take (below): the .break lines, but no .seq
 *     line, because the sums are the caller's; the group's row gets PTEXT_HOST_SEQ and the caller splices its own line in
 *     at seq_off of the row.
 * The formatter takes +-0 and every finite double with 2^-64 <= |x| < 2^64, which covers every average of a group that
 * eval_groups* did not flag (0, or in [2^-63, 2^31]), and declines everything else: NaN, the infinities, denormals.
 * Nothing is written for a missing line, and every byte of either text belongs to exactly one line: the lines lie one
 * after the other in group order, the offsets of the line table are the 64-bit running sums of the lengths (a missing
 * line has length 0 and the offset of the next one), and either text may pass 2^31 bytes.
 *
 * Plain C types; host pointers unless the name says _device.  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: creating an object fails with DSA_E_DEVICE without a GPU.  Argument errors that can
 * be told from the arguments alone are found before a device is touched.  One object must not be used from two threads at
 * once.  Out of scope: the tools (they keep their host formatters), the NaN and infinity texts of EVAL_HOST_STATS groups,
 * more than one GPU per chain, a streamed entry, locales other than C.
 *
 * A second section, "span statistics" (span_*), follows at the end: splitreads.span.stats from the same prediction and the
 * cluster text of a taskc_ctx.
 */
#ifndef DEFUSE_PTEXT_H_
#define DEFUSE_PTEXT_H_

#include <stdint.h>

#include "defuse_dsa.h"
#include "defuse_pred.h"
#include "defuse_task.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTEXT_HOST_SEQ  16  /* or-ed into the group's EVAL_* / PRED_* bits: .break lines, and the .seq line is the caller's */

/* The reference name and align strand of one cluster end of one fusion. */
typedef struct ptext_end {
    int32_t fusion_id;
    int32_t cluster_end;               /* 0 / 1                                                                        */
    int32_t name;                      /* mAlignRefName is name_bytes[name_off[name] .. name_off[name + 1])            */
    int32_t strand;                    /* mAlignStrand: 0 = PlusStrand, 1 = MinusStrand                                */
} ptext_end;

/* One group's lines: the .seq line is seq_text[seq_off .. seq_off + seq_len), the two .break lines together are
 * brk_text[brk_off .. brk_off + brk_len).  A length of 0: the group has no such line. */
typedef struct ptext_line {
    int64_t seq_off;
    int64_t seq_len;                   /* (a sequence of 2^31 - 1 bytes makes a longer line)                           */
    int64_t brk_off;
    int64_t brk_len;
    int32_t status;                    /* the group's EVAL_* and PRED_* bits, or-ed with PTEXT_HOST_SEQ                */
    int32_t pad_;
} ptext_line;

/* The texts of the latest ptext_format of a ctx on the device.  Valid until the next ptext_format on the ctx or its
 * destruction. */
typedef struct ptext_device_view {
    const void* seq_text;              /* device pointers, never NULL after a successful call                          */
    const void* brk_text;
    const void* lines;                 /* ptext_line[n_lines]                                                          */
    int64_t seq_text_len;
    int64_t brk_text_len;
    int64_t n_lines;
    int32_t device;
    int32_t pad_;
} ptext_device_view;

/* HIP-event times of the most recent ptext_format of a ctx, and of the most recent ptext_fetch after it. */
typedef struct ptext_timing {
    float   lengths_ms;                /* the line lengths, the two 64-bit sums, the totals to the host                */
    float   write_ms;                  /* heads, tails, all .break bytes, the line table, the copy descriptors         */
    float   gather_ms;                 /* the sequences into the .seq text                                             */
    float   download_ms;               /* ptext_fetch                                                                  */
    int64_t n_groups;
    int64_t seq_text_bytes;
    int64_t brk_text_bytes;
    int64_t gather_bytes;              /* bytes of the .seq text that the gather wrote                                 */
} ptext_timing;

typedef struct ptext_names ptext_names;     /* opaque: the names and align strands of a run on one device         */
typedef struct ptext_ctx ptext_ctx;         /* opaque: the output buffers of one caller, reused call after call   */

/* The name table of a run and its cluster ends, in any order; everything is copied, the caller's buffers are free on
 * return.  name_off has n_names + 1 ascending offsets into name_bytes; an empty name is allowed.  DSA_E_ARG, naming the
 * record, for a name that begins below 0, ends before it begins or ends outside name_bytes, for an end with a cluster_end
 * or a strand other than 0 / 1 or a name outside the table, and for two ends with one (fusion_id, cluster_end).
 * n_names = 0 and n_ends = 0 are allowed. */
int ptext_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names,
                       const ptext_end* ends, int64_t n_ends, ptext_names** out);
void ptext_names_destroy(ptext_names* names);

int ptext_create(int device, ptext_ctx** out);
void ptext_destroy(ptext_ctx* ctx);

/* Both texts and one ptext_line per group of the latest pred_predict* of `pred`, left on the device in the buffers of
 * `ctx`, which grow as needed and are kept.  `pred` is read in place and must not run a prediction during the call.  After
 * a failure both texts and the line table are empty.  DSA_E_ARG: an object is missing, the objects are not on one device,
 * `pred` has no completed prediction (none yet, or its latest call failed), or a group that gets lines has a cluster end
 * without an entry in `names`; the error names the lowest such group. */
int ptext_format(ptext_ctx* ctx, const pred_ctx* pred, const ptext_names* names);

int ptext_view(const ptext_ctx* ctx, ptext_device_view* out);
/* Downloads the two texts and the line table (a buffer whose capacity is 0 may be NULL).  DSA_E_CAPACITY if one of them
 * does not fit; nothing is written then.  Capacities are in elements: bytes, bytes, ptext_line. */
int ptext_fetch(ptext_ctx* ctx, uint8_t* seq_text, int64_t seq_cap, uint8_t* brk_text, int64_t brk_cap, ptext_line* lines, int64_t lines_cap);
int ptext_get_timing(const ptext_ctx* ctx, ptext_timing* out);

/* The "%g" texts of x[0 .. n) as the device build of the formatter prints them, back to back in out[0 .. *out_len);
 * len[k] is the length of the k-th text, 0 where the formatter declines.  *out_len always receives the total on success
 * and on DSA_E_CAPACITY (total > cap; out and len are not written then).  DSA_E_LIMIT: n > 2^30 - 1. */
int ptext_format_doubles(int device, const double* x, int64_t n, uint8_t* out, int64_t cap, int32_t* len, int64_t* out_len);

const char* ptext_last_error(void);

/* ---- span statistics ----------------------------------------------------------------------------------------------------
 *
 * splitreads.span.stats, the file scripts/calc_span_stats.pl makes right after evalsplitalign from clusters.sc,
 * splitreads.break and splitreads.seq: per cluster the mean length of its spanning fragments up to the predicted break,
 * and their number.  In a chain run both inputs are in device memory already: the de-duplicated cluster text in a taskc_ctx
 * (defuse_task.h, "cluster text"), the break positions in a pred_ctx.
 *
 * Three maps, in each the last line of a key wins:
 *     .break lines    break[(id, end)] = field 4        (fields 0, 1)
 *     .seq lines      inter[id] = field 2               (field 0; WriteSequence prints 0 there)
 *     cluster lines   strand[(id, end)] = field 5 of the last line of that (id, end), whatever its fragment;
 *                     pos[(id, fragment, end)] = fields 6 and 7 of the last line of that triple (the winner)
 * Rows, for every id of the cluster text that has any break entry (the others are skipped, whatever they are made of):
 *     - the id has exactly two distinct cluster ends among its lines;
 *     - every distinct fragment's length is the sum of one term per end THE FRAGMENT HAS, break - start + 1 if
 *       strand[(id, end)] is exactly "+", else end - break + 1 (only the one position field the strand selects is read),
 *       plus inter[id], once per fragment;
 *     - sum = the sum over the fragments (an int64), count = their number, mean = (double)sum / (double)count;
 *     - the text line "%d\t%.15g\t%lld\n" of id, mean, count: what Perl prints for the quotient while |sum| <= 2^53.
 * Ids, ends and fragments are ints as in the cluster text section: "+7", "007" and "7" are one value, an id prints in plain
 * decimal, groups are over the whole text, rows ascend by id (the script: hash order).  n_noncanonical counts the key fields
 * (cluster fields 0, 1, 2; .break fields 0, 1; .seq field 0) that are not byte for byte the "%d" of their value: where it
 * is 0, Perl's string keys and these int keys are the same keys.
 *
 * Stops end a call with DSA_OK and a filled result, and the ctx then holds no output of that call's kind.
 *   Line stops, the lowest line of the file in question (.break before .seq in span_breaks_text): fewer than 8 / 5 / 3 fields
 *   in a cluster / .break / .seq line is SPAN_FEW_FIELDS; cluster fields 0, 1, 2, .break fields 0, 1, 4 and .seq fields 0, 2
 *   are integers (optional sign, digits, int range; "1e2", " 349" and "12\r" are none), else SPAN_BAD_INTEGER with the first
 *   such field.  stop_line is 1-based in the text looked at (for TASKC_DEDUP the dedup text), stop_file says which.
 *   Id stops, only for ids with a break entry, the lowest id as int, stop_line 0, stop_value the id; within one id the first of
 *     SPAN_NOT_TWO_ENDS   not exactly two distinct cluster ends;
 *     SPAN_NO_BREAK_END   a winner's (id, end) has no break entry;
 *     SPAN_BAD_INTEGER    the position field a winner uses is no integer (stop_field 6 or 7, the lower if both occur);
 *     SPAN_COORD_LIMIT    a break a winner uses, a position a winner uses, or the id's inter is beyond +-TASK_MAX_COORD,
 *                         which keeps every sum inside an int64;
 *     SPAN_NO_INTER       the id has no inter entry;
 *     SPAN_SUM_LIMIT      |sum| > 2^53.
 *   A line stop beats an id stop.
 */
#define SPAN_FEW_FIELDS     1
#define SPAN_BAD_INTEGER    2
#define SPAN_NOT_TWO_ENDS   3
#define SPAN_NO_BREAK_END   4
#define SPAN_COORD_LIMIT    5
#define SPAN_NO_INTER       6
#define SPAN_SUM_LIMIT      7
#define SPAN_FILE_CLUSTERS  0      /* stop_file                                                                       */
#define SPAN_FILE_BREAKS    1
#define SPAN_FILE_SEQS      2

typedef struct span_result {
    int64_t n_lines;                   /* span_stats: cluster lines; span_breaks_text: .break lines; _pred: groups     */
    int64_t n_seq_lines;               /* span_breaks_text: .seq lines                                                 */
    int64_t n_breaks;                  /* span_breaks_*: distinct (id, end) of the break table                         */
    int64_t n_inters;                  /* span_breaks_*: distinct ids of the inter table                               */
    int64_t n_ids;                     /* span_stats: distinct ids of the cluster text                                 */
    int64_t n_rows;                    /* span_stats: ids with a break entry                                           */
    int64_t out_bytes;                 /* span_stats: bytes of the text                                                */
    int64_t n_noncanonical;            /* key fields of this call's texts that are not their "%d"                      */
    int64_t stop_line;                 /* 1-based; 0: no stop, or an id stop                                           */
    int64_t stop_value;                /* an id stop: the id                                                           */
    int32_t stop_kind;                 /* SPAN_*, 0: no stop                                                           */
    int32_t stop_field;                /* SPAN_BAD_INTEGER: the field, else -1                                         */
    int32_t stop_file;                 /* SPAN_FILE_*; meaningful with a stop                                          */
    int32_t pad_;
} span_result;

typedef struct span_row {
    int32_t cluster_id;
    int32_t text_len;                  /* the row's line is text[text_off .. text_off + text_len)                      */
    int64_t text_off;
    int64_t count;                     /* distinct fragments                                                           */
    int64_t sum;
    double  mean;
} span_row;

/* The output of the latest span_stats of a ctx on the device; valid until the next call on the ctx or its destruction. */
typedef struct span_device_view {
    const void* rows;                  /* span_row[n_rows], ascending cluster_id; device pointers, never NULL          */
    const void* text;
    int64_t n_rows;
    int64_t text_len;
    int32_t device;
    int32_t pad_;
} span_device_view;

/* HIP-event times of the most recent span_breaks_*, span_stats and span_fetch of a ctx. */
typedef struct span_timing {
    float   upload_ms;                 /* span_breaks_text: both texts to the device                                   */
    float   lines_ms;                  /* span_breaks_*: line and tab tables and the line rules, or the pass over pred */
    float   tables_ms;                 /* span_breaks_*: the two sorts, the last of each run                           */
    float   sorts_ms;                  /* span_stats: keys, the two sorts, groups and strands                          */
    float   terms_ms;                  /* span_stats: winners, lookups, terms, the sums, the rows' rules               */
    float   print_ms;                  /* span_stats: offsets, rows and text                                           */
    float   download_ms;               /* span_fetch                                                                   */
    float   pad_;
    int64_t n_lines;                   /* cluster lines of the latest span_stats                                       */
    int64_t n_rows;
} span_timing;

typedef struct span_ctx span_ctx;      /* opaque: the two tables and the output of one caller, reused call after call  */

int span_create(int device, span_ctx** out);
void span_destroy(span_ctx* ctx);

/* The two files as text, each whole (a last line without a newline is a line).  DSA_E_ARG for a negative length or a null
 * pointer with a length, DSA_E_LIMIT for more than 2^31 - 1 bytes in either.  Leaves the sorted (id, end) -> break table and
 * the id -> inter table on the device, replacing the ones before; after a stop or a failure the ctx has no tables. */
int span_breaks_text(span_ctx* ctx, const uint8_t* brk_text, int64_t brk_len, const uint8_t* seq_text, int64_t seq_len, span_result* result);
/* The same tables from the latest successful prediction of `pred`, read in place: for every group that gets .break lines
 * (neither PRED_NO_TASK nor PRED_OUT_OF_WINDOW) two break entries with the position its .break lines carry (0 for a group
 * without a split) and inter 0, PTEXT_HOST_SEQ groups included, whose .seq line carries the same 0.  DSA_E_ARG if an object
 * is missing, the two are not on one device, or `pred` has no completed prediction. */
int span_breaks_pred(span_ctx* ctx, const pred_ctx* pred, span_result* result);
/* Rows and text over the cluster text of `clusters`: source TASKC_INPUT (the text as added) or TASKC_DEDUP (the output of
 * its last taskc_dedup); the line records taskc parsed are reused.  DSA_E_ARG for another source, a missing object, objects
 * on two devices, a ctx without tables, or TASKC_DEDUP without a dedup text. */
int span_stats(span_ctx* ctx, taskc_ctx* clusters, int32_t source, span_result* result);

/* DSA_E_ARG if the ctx has no output (no span_stats yet, or its latest one stopped or failed). */
int span_view(const span_ctx* ctx, span_device_view* out);
/* Downloads rows and text (a buffer whose capacity is 0 may be NULL; capacities in elements).  DSA_E_CAPACITY if either does
 * not fit; nothing is written then. */
int span_fetch(span_ctx* ctx, span_row* rows, int64_t rows_cap, uint8_t* text, int64_t text_cap);
int span_get_timing(const span_ctx* ctx, span_timing* out);

/* The "%.15g" texts of x[0 .. n) as the device build of the formatter prints them, back to back in out[0 .. *out_len);
 * len[k] is the length of the k-th text, 0 where the formatter declines (it takes +-0 and 2^-64 <= |x| < 2^64).  *out_len
 * receives the total on success and on DSA_E_CAPACITY (total > cap; out and len are not written then).  DSA_E_LIMIT:
 * n > 2^30 - 1. */
int span_format_doubles(int device, const double* x, int64_t n, uint8_t* out, int64_t cap, int32_t* len, int64_t* out_len);

const char* span_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
