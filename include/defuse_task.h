/*
 * defuse_task.h — C ABI of the MI355X task creation in front of the resident split-read chain ("task").
 *
 * Replaces, for all fusions of a run at once, CreateTasks / SplitAlignmentTask::Initialize:
 *
 *     CalculateBreakRegion, the two windows      tools/SplitAlignment.cpp:61-79, :637-655   -> task_store_create, the plan
 *     the two remainders                         tools/SplitAlignment.cpp:81-104            -> task_store_create, the plan
 *     FastaIndex::Get and its clipping           tools/FastaIndex.cpp:23-61, faidx.c:305-357 -> the plan and the two gathers
 *     RemapTranscriptToGenome, the mate region   tools/SplitAlignment.cpp:106-145            -> the plan
 *     GetRegionTranscripts                       tools/ExonRegions.cpp:131-161               -> the region kernel
 *     RemapThroughTranscript                     tools/ExonRegions.cpp:421-482               -> the region kernel
 *
 * It is the first link of the resident chain: the integers of the regions file go up, and the windows, remainders and mate
 * regions of every task are made on the device.  The store hands out a bat_windows and a pred_tasks that bat_assemble* and
 * pred_predict* read in place; no host copy of the windows is made and there is no second device copy of them.
 *
 * task_store_create leaves the strings with the caller, who resolves every name to a dense index once: sequences of the
 * FASTA (task_seq), chromosomes and transcripts of the exon table, and the reference numbering of cand_region.ref.  The
 * section "region and exon text" at the end takes the regions file and the exon table as text instead and resolves the names
 * on the device.
 *
 * FastaIndex::Get, exactly (start and length are its int& parameters):
 *   - length < 0: returns the empty string before the name is looked at; start and length stay as they are;
 *   - start < 1: length -= 1 - start, start = 1; end = start + length - 1;
 *   - the name is looked up ("Unable to find sequence for": TASK_NO_SEQUENCE_* if the end's seq is -1);
 *   - beg = start - 1, clipped to the sequence length; an end below 0 or at or beyond the sequence length becomes the sequence
 *     length (faidx compares the int with an unsigned field: a window that lies wholly in front of the sequence returns the
 *     whole sequence); beg > end collapses to end; length = end - beg;
 *   - on the minus strand the bytes are reversed and A<->T, C<->G exchanged in either case, every other byte kept
 *     (tools/Common.cpp:32-54).
 * The clipped start and length are seq_start / seq_len of the record and flow into the remainder's Get.
 *
 * Mate regions (cand_region[], what cand_table_create takes): task by task in input order, end 0 before end 1; within an end
 * the genomic region first (ref = chrom_ref of the end's chromosome, or of its transcript's chromosome for an end that names
 * a transcript), then one region per overlapping transcript whose RemapThroughTranscript succeeds, in ascending transcript
 * index, with ref = the transcript's name_ref.  id = ClusterID(fusion_id, end).  The overlapping transcripts are found as the reference
 * finds them: bins of 100000 with C++ int division over (first exon's start, last exon's end), the inclusive overlap test on
 * each entry, each transcript once.
 *
 * Limits (DSA_E_LIMIT, naming the record).  The reference computes in int; inside these bounds no intermediate leaves int32:
 *   - every coordinate (align start / end, exon start / end) in [-TASK_MAX_COORD, TASK_MAX_COORD];
 *   - |end - start + 1| of an align region <= TASK_MAX_REGION;
 *   - min_fragment and max_fragment in [-TASK_MAX_PARAM, TASK_MAX_PARAM], min_read and max_read in [0, TASK_MAX_PARAM];
 *   - the sum over a transcript's exons of |end - start + 1| <= TASK_MAX_COORD;
 *   - a sequence of the reference has at most TASK_MAX_SEQ_LEN bytes;
 *   - a window longer than dsa_limits.max_ref_len (the faidx quirk can return a whole chromosome), more than 2^31 - 1 window
 *     bytes in all (the offsets of bat_windows are int32), more than 2^31 - 1 mate regions.  Remainder offsets are 64-bit.
 *
 * Plain C types; host pointers unless the name says _device.  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: creating an object fails with DSA_E_DEVICE without a GPU.  Argument errors that can
 * be told from the arguments alone are found before a device is touched.  One object must not be used from two threads at
 * once.  Out of scope: the tools (they keep host CreateTasks and the task cache), sharing bytes with la_genome, a
 * cand_table_create from device regions, reading FASTA / .fai, more than one GPU per chain.
 */
#ifndef DEFUSE_TASK_H_
#define DEFUSE_TASK_H_

#include <stdint.h>

#include "defuse_bat.h"
#include "defuse_cand.h"
#include "defuse_dsa.h"
#include "defuse_pred.h"
#include "defuse_sc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TASK_MAX_COORD    (1 << 28)
#define TASK_MAX_REGION   (1 << 24)
#define TASK_MAX_PARAM    (1 << 20)
#define TASK_MAX_SEQ_LEN  (1 << 30)
#define TASK_EXON_BIN     100000       /* tools/ExonRegions.cpp:19 */

/* task_record.status: one bit per end and cause, in the order the reference meets them; the lowest set bit is the message it
 * would have printed before it exits.  A flagged task's other fields are unspecified. */
#define TASK_NO_SEQUENCE_0     1   /* "Error: Unable to find sequence for <end 0's name>"                               */
#define TASK_BAD_CHROMOSOME_0  2   /* "Error: Data mismatch, invalid chromosome <end 0's name>"                         */
#define TASK_NO_SEQUENCE_1     4
#define TASK_BAD_CHROMOSOME_1  8

/* One sequence of the FASTA: its graph characters, as given, are bytes[off .. off + len). */
typedef struct task_seq {
    int64_t off;
    int64_t len;
} task_seq;

/* One line of the exon table. */
typedef struct task_transcript {
    int32_t chrom;                     /* index into chrom_ref                                                         */
    int32_t strand;                    /* 0 / 1                                                                        */
    int32_t first_exon;                /* its exons are exons[first_exon .. first_exon + n_exons), in file order       */
    int32_t n_exons;                   /* >= 1                                                                         */
    int32_t name_ref;                  /* cand_region.ref of "gene|transcript", >= 0                                   */
} task_transcript;

typedef struct task_exon {
    int32_t start, end;
} task_exon;

typedef struct task_params {
    int32_t min_fragment;              /* (int)(mean - 3 sd)                                                           */
    int32_t max_fragment;              /* (int)(mean + 3 sd)                                                           */
    int32_t min_read;
    int32_t max_read;
} task_params;

/* One align region of the regions file. */
typedef struct task_end {
    int32_t seq;                       /* sequence index of its name in the reference, -1: the FASTA has no such name  */
    int32_t transcript;                /* transcript index if ParseTranscriptID && IsTranscript, else -1               */
    int32_t chrom;                     /* chromosome index of the exon table if the name is one, else -1               */
    int32_t strand;                    /* 0 / 1                                                                        */
    int32_t start, end;
} task_end;

typedef struct task_pair {
    int32_t fusion_id;                 /* in [0, 2^31), distinct                                                       */
    task_end end[2];
} task_pair;

/* One task, as SplitAlignmentTask::Initialize leaves it; index 0 / 1 is the cluster end. */
typedef struct task_record {
    int32_t fusion_id;
    int32_t status;                    /* TASK_* bits, 0: the reference creates this task                              */
    int32_t seq_start[2];              /* mSplitAlignSeqStart, after Get                                               */
    int32_t seq_len[2];                /* mSplitAlignSeqLength, after Get; the window has max(seq_len, 0) bytes        */
    int32_t seq_strand[2];             /* mSplitSeqStrand                                                              */
    int32_t win_off[2];                /* the window is window_bytes[win_off .. win_off + max(seq_len, 0))             */
    int32_t rem_len[2];                /* mSplitRemainderSeq is rem_bytes[rem_off .. rem_off + rem_len)                */
    int64_t rem_off[2];
    int32_t n_regions[2];              /* mMateRegions[end] is regions[region_off (+ n_regions[0]) ...)                */
    int64_t region_off;
} task_record;

typedef struct task_counts {
    int64_t n_tasks;
    int64_t window_bytes;
    int64_t rem_bytes;
    int64_t n_regions;
} task_counts;

/* HIP-event times of task_store_create, and of the most recent task_store_fetch. */
typedef struct task_timing {
    float   upload_ms;                 /* the pairs to the device                                                      */
    float   plan_ms;                   /* break regions, cuts, genome walk, genomic mate region, status                */
    float   count_ms;                  /* the overlapping transcripts of every end, counted                            */
    float   scan_ms;                   /* the three sums and their totals to the host                                  */
    float   region_ms;                 /* the regions emitted, the records and the gathers' descriptors written        */
    float   gather_ms;                 /* the two gather launches: windows, then remainders                            */
    float   sort_ms;                   /* the key order of bat_windows / pred_tasks                                    */
    float   download_ms;               /* task_store_fetch                                                             */
    int64_t n_tasks;
    int64_t n_regions;
    int64_t window_bytes;
    int64_t rem_bytes;
} task_timing;

typedef struct task_reference task_reference;   /* opaque: the sequences of the FASTA on one device    */
typedef struct task_exons task_exons;           /* opaque: the exon table on one device                */
typedef struct task_store task_store;           /* opaque: the tasks of a run on one device            */

/* The bytes are copied once; the caller's buffers are free on return.  DSA_E_ARG, naming the sequence, for one outside
 * bytes; DSA_E_LIMIT for one longer than TASK_MAX_SEQ_LEN.  n_seqs = 0 is allowed. */
int task_reference_create(int device, const uint8_t* bytes, int64_t bytes_len, const task_seq* seqs, int64_t n_seqs,
                          task_reference** out);
void task_reference_destroy(task_reference* reference);

/* chrom_ref[c] is the cand_region.ref a mate region on chromosome c gets.  The transcript index order is the output order
 * of the regions: ascending transcript names give the reference's.  DSA_E_ARG, naming the transcript, for one without exons
 * (the reference reads no such line), exons outside the table, a chromosome outside chrom_ref, a strand other than 0 / 1, a
 * negative name_ref. */
int task_exons_create(int device, const int32_t* chrom_ref, int32_t n_chroms, const task_transcript* transcripts,
                      int32_t n_transcripts, const task_exon* exons, int64_t n_exons, task_exons** out);
void task_exons_destroy(task_exons* exons);

/* All tasks of a run.  reference and exons are on `device` and may be destroyed once the call returns: the store keeps
 * nothing of them.  Several stores may be made from one reference and one exon table.  DSA_E_ARG, naming the pair, for a
 * fusion_id below 0, two pairs with one fusion_id, a strand other than 0 / 1, an index below -1 or beyond its table.  n = 0
 * is allowed. */
int task_store_create(const task_reference* reference, const task_exons* exons, const task_params* params,
                      const task_pair* pairs, int64_t n, task_store** out);
/* After every bat_batch / pred_ctx call that uses its windows or tasks has returned; those objects may be destroyed before
 * or after the store. */
void task_store_destroy(task_store* store);

/* Both windows of every task, keyed by fusion_id ascending as unsigned: what bat_windows_create returns, owned by the store
 * (never given to bat_windows_destroy) and valid as long as it lives. */
const bat_windows* task_store_windows(const task_store* store);
/* Likewise what pred_tasks_create returns over task_store_windows. */
const pred_tasks* task_store_pred_tasks(const task_store* store);

int task_store_counts(const task_store* store, task_counts* out);
/* Downloads the task records (input order), both byte pools and the regions; a part whose buffer is NULL (with capacity 0)
 * is left where it is, so that a caller who only needs the records and the regions moves no window bytes.  DSA_E_CAPACITY if
 * a part that is asked for does not fit (task_store_counts says what is needed); nothing is written then.  Capacities are in
 * elements. */
int task_store_fetch(task_store* store, task_record* records, int64_t records_cap, uint8_t* window_bytes, int64_t window_cap,
                     uint8_t* rem_bytes, int64_t rem_cap, cand_region* regions, int64_t regions_cap);
int task_store_get_timing(const task_store* store, task_timing* out);

const char* task_last_error(void);

/* ---- region and exon text ------------------------------------------------------------------------------------------------
 *
 * The regions file (ReadAlignRegionPairs, tools/Parsers.cpp:211-264) and the exon table (ExonRegions::Read,
 * tools/ExonRegions.cpp:21-112) go up as text; the lines are split, the integers read, the names sorted and looked up and the
 * pairs made on the device, where taskt_store_create hands them to the kernels of task_store_create.  The pairs never come
 * down unless taskt_pairs_fetch asks for them.
 *
 * Text, both files: lines end at '\n'; only '\n' and '\t' are special, a '\r' belongs to its field; a last line without a
 * newline is a line; empty text has no line.  An integer is what boost::lexical_cast<int> reads: an optional sign, digits
 * only, inside int ("+007" and "7" are one value, "+", "" and 2147483648 are none).  A text of more than 2^31 - 1 bytes is
 * DSA_E_LIMIT.  Names are compared byte by byte as unsigned bytes; nothing is hashed.
 *
 * A stop ends the stream where the reference's exit(1) does: the result names the first line in file order that has any
 * cause (stop_line, 1-based; stop_off / stop_len, its bytes without the newline, so that the caller can print the reference's
 * message), the cause and its field; the other counts of the result are those of the lines in front of it or zero, as said
 * below.  The call returns DSA_OK.  After a stop the ctx holds no table of that kind, and the calls that need one return
 * DSA_E_ARG.
 *
 * Exon table, per line, in this order:
 *   (1) length 0 or fewer than six fields: skipped (counted in n_skipped);
 *   (2) fields (4, 5), (6, 7), ... are exons: the reference's loop runs k = 5; k < n_fields; k += 2, so a last unpaired field
 *       is never looked at.  The first member of a pair that is no integer stops (TASKT_EXON_BAD_INTEGER, "Failed to
 *       interpret exon:"); "g\tt\tc\t+\t1\t" has six fields and stops on field 5;
 *   (3) field 3 is "+" or "-", else TASKT_EXON_BAD_STRAND ("Error: Unable to intepret strand");
 *   (4) limits of this library, where the reference reads on (kinds >= TASKT_LIBRARY_LIMIT): field 1 (the transcript) or
 *       field 2 (the chromosome) longer than TASKT_MAX_NAME bytes is TASKT_EXON_LONG_NAME with that field; a transcript
 *       name that an earlier transcript line has is TASKT_EXON_DUPLICATE (field 1) on the later line (the reference
 *       overwrites its maps and keeps the old bins, which an index-based table cannot say).
 * The table: transcripts are numbered in ascending byte order of field 1, a prefix first (what task_exons_create wants for
 * the reference's output order); the exons stay in file order, those of a transcript side by side; chromosomes are numbered
 * by first appearance.  chrom_ref[c] is the position of the chromosome's name in ref_names, name_ref the position of the
 * bytes gene + "|" + transcript; a name ref_names does not have gets n_names + c, or n_names + n_chroms + t for transcript t
 * (every region has a ref, and no SAM line can match an absent name).  DSA_E_LIMIT if those numbers leave int32.  The
 * derived columns and the checks of the table itself are task_exons_create's, with its codes and messages.
 *
 * Regions file, per line, in this order:
 *   (1) length 0 or fewer than five fields: skipped;
 *   (2) fields 0 and 1 are integers, else TASKT_REGION_BAD_INTEGER with the field ("Failed to interpret region:");
 *   (3) field 1 is 0 or 1, else TASKT_REGION_BAD_END ("Error: DebugCheck pairEnd == 0 || pairEnd == 1 failed");
 *   (4) field 3 is "+" or "-", else TASKT_REGION_BAD_STRAND;
 *   (5) a line of exactly five fields is TASKT_REGION_BAD_INTEGER on field 5; fields 4 and 5 are integers, else the same
 *       with their field.  Further fields are ignored.
 * The pairs: one per distinct id, ascending (as int); per (id, end) the last line of the file wins; an end no line gives is
 * the default Location (empty name, strand 0, start 0, end 0).  Every end, the default one too, is resolved: seq is the
 * position of the whole name in seq_names or -1; transcript the index of the second '|'-separated field if the name has at
 * least two and the exon table has that transcript, else -1 ("g|t|x" gives t, "g|" the empty name); chrom the index of the
 * whole name among the exon table's chromosomes or -1.
 *
 * seq_names: position = the task_seq index of the caller's task_reference.  ref_names: position = the cand_region.ref
 * numbering the caller's SAM parse uses.  They may be one object.  One ctx must not be used from two threads at once. */

#define TASKT_MAX_NAME            64
#define TASKT_EXON_BAD_INTEGER    1
#define TASKT_EXON_BAD_STRAND     2
#define TASKT_REGION_BAD_INTEGER  3
#define TASKT_REGION_BAD_END      4
#define TASKT_REGION_BAD_STRAND   5
#define TASKT_LIBRARY_LIMIT       16
#define TASKT_EXON_LONG_NAME      16
#define TASKT_EXON_DUPLICATE      17

typedef struct taskt_result {
    int64_t n_lines;                   /* lines of the text; with a stop, the lines in front of it                     */
    int64_t n_skipped;                 /* of them skipped by rule (1); 0 with a stop                                   */
    int64_t n_items;                   /* transcripts of the table / pairs of the regions file; 0 with a stop          */
    int64_t n_exons;                   /* exon table only                                                              */
    int64_t n_chroms;                  /* exon table only                                                              */
    int64_t name_bytes;                /* exon table only: the bytes of all transcript names (field 1)                 */
    int64_t stop_line;                 /* 1-based, 0: no stop                                                          */
    int64_t stop_off, stop_len;        /* the stopping line is text[stop_off .. stop_off + stop_len)                   */
    int32_t stop_kind;                 /* TASKT_*                                                                      */
    int32_t stop_field;                /* the field that stopped, -1 without a stop                                    */
} taskt_result;

/* HIP-event times of the most recent call of each kind; exon_table_ms is the rest of taskt_parse_exons by a host clock. */
typedef struct taskt_timing {
    float   exon_upload_ms;            /* the exon text to the device                                                  */
    float   exon_device_ms;            /* tables, line rules, exon emit, the two name sorts, the lookups               */
    float   exon_table_ms;             /* the arrays down, task_exons_create, the call's allocations                   */
    float   region_upload_ms;
    float   region_device_ms;          /* tables, line rules, the sort by (id, end), the lookups, the pairs            */
    float   check_ms;                  /* taskt_store_create: the pairs' checks (the rest is task_timing's)            */
    int64_t exon_bytes;
    int64_t region_bytes;
} taskt_timing;

typedef struct taskt_names taskt_names;         /* opaque: a list of names on one device               */
typedef struct taskt_ctx taskt_ctx;             /* opaque: buffers, the exon table and the pairs       */

/* Name k is name_bytes[name_off[k] .. name_off[k + 1]): name_off has n_names + 1 ascending entries.  The bytes are copied.
 * DSA_E_ARG for offsets outside the bytes or descending, and for two equal names (naming both).  The contract of the text
 * front's names table (defuse_text.h). */
int taskt_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names,
                       taskt_names** out);
void taskt_names_destroy(taskt_names* names);

int taskt_create(int device, taskt_ctx** out);
void taskt_destroy(taskt_ctx* ctx);

/* The whole exon table (cdna.regions) as one text.  Replaces the ctx's exon table and drops its pairs.  ref_names may be
 * destroyed once the call returns. */
int taskt_parse_exons(taskt_ctx* ctx, const taskt_names* ref_names, const uint8_t* text, int64_t len, taskt_result* result);
/* The whole regions file as one text.  DSA_E_ARG if the ctx has no exon table.  Replaces the ctx's pairs.  seq_names may be
 * destroyed once the call returns. */
int taskt_parse_regions(taskt_ctx* ctx, const taskt_names* seq_names, const uint8_t* text, int64_t len, taskt_result* result);

/* What task_exons_create returns for the parsed table, owned by the ctx (never given to task_exons_destroy) and valid until
 * the next taskt_parse_exons or taskt_destroy; NULL if there is none. */
const task_exons* taskt_exons(const taskt_ctx* ctx);
/* The parsed table: transcripts[t] and chrom_ref as task_exons_create took them, the exons in file order, and the name of
 * transcript t as name_bytes[name_off[t] .. name_off[t + 1]) (name_off has n_items + 1 entries).  A part whose buffer is NULL
 * (with capacity 0) is left out; DSA_E_CAPACITY if a part that is asked for does not fit (the result of taskt_parse_exons
 * says what is needed).  Capacities are in elements. */
int taskt_exons_fetch(taskt_ctx* ctx, task_transcript* transcripts, int64_t transcripts_cap, task_exon* exons, int64_t exons_cap, int32_t* chrom_ref,
                      int64_t chrom_cap, int64_t* name_off, int64_t name_off_cap, uint8_t* name_bytes, int64_t name_bytes_cap);
/* The pairs, for tests and callers who want them; lines[2 * k + e], if given, is the 1-based line that gave pair k its end e,
 * 0 for a default end. */
int taskt_pairs_fetch(taskt_ctx* ctx, task_pair* pairs, int64_t pairs_cap, int64_t* lines, int64_t lines_cap);

/* task_store_create over the ctx's exon table and pairs, which stay on the device: a task_store, used and destroyed through
 * the store functions above.  seq_names of the regions parse must not have more names than the reference has sequences
 * (DSA_E_ARG).  The pairs' checks are made on the device and name the lowest offending pair by index, fusion id and line:
 * DSA_E_ARG for a negative fusion id, DSA_E_LIMIT for a coordinate beyond TASK_MAX_COORD, a span beyond TASK_MAX_REGION and
 * more than 2^30 - 1 pairs. */
int taskt_store_create(taskt_ctx* ctx, const task_reference* reference, const task_params* params, task_store** out);

int taskt_get_timing(const taskt_ctx* ctx, taskt_timing* out);
const char* taskt_last_error(void);

/* ---- cluster text ------------------------------------------------------------------------------------------------------
 *
 * The two steps between the set cover and the regions parse, on cluster text that is in device memory or goes there in
 * pieces: what `defuse_glue remove_duplicates MIN` prints (scripts/remove_duplicates.pl), what `defuse_glue
 * get_align_regions` prints (scripts/get_align_regions.pl), and the pairs of a taskt_ctx made from that regions text where
 * it lies.  The text comes down only if taskc_fetch asks for it.
 *
 * Text: lines end at '\n'; a '\r' belongs to its field; a last line without a newline is a line; empty text has no line.
 * Only the first eight tab-separated fields matter: cluster id, cluster end, fragment, read end, name, strand, start, end.
 * Field 7 ends at the eighth tab or at the line's end; later fields are ignored.  An integer is an optional sign and digits
 * only, inside int ("7", "+7" and "007" are one value).
 *
 * Dedup, per line, in this order:
 *   (1) fewer than eight fields: TASKC_FEW_FIELDS (an empty line is one);
 *   (2) fields 0, 1 and 2 are integers, else TASKC_BAD_INTEGER with the first such field;
 *   (3) a cluster end other than 0 or 1: the line belongs to its run (it can begin, continue or separate runs) but carries no
 *       fragment, and nothing more of it is checked;
 *   (4) the position field is 6 if field 5 is exactly "+", else 7; it is an integer, else TASKC_BAD_INTEGER with that field.
 *       The other of the two is never looked at.
 * Dedup, per run (a maximal sequence of adjacent lines whose field 0 has one int value; an id that comes back later is a new
 * run): per (fragment, cluster end) the last line in file order wins; a fragment with only one of its ends is
 * TASKC_MISSING_END, attributed to the run's last line, stop_value the lowest such fragment; the fragments are ordered by
 * (position of end 0, position of end 1, fragment) as int and the first of every distinct position pair is kept; the run is
 * printed iff the kept fragments number at least min_cluster_size (a signed 64-bit compare: 0 or less keeps every run).
 * Output: runs in file order, kept fragments ascending, per fragment the winning end-0 line, then the winning end-1 line,
 * each the input's bytes and '\n'.
 *
 * Regions, per line: fewer than eight fields is TASKC_FEW_FIELDS; fields 0, 1, 6 and 7 are integers, checked in that order,
 * else TASKC_BAD_INTEGER with the field.  Groups are (id, cluster end) over the whole text, any int as cluster end: name and
 * strand are the bytes of fields 4 and 5 of the group's last line, start the least field 6, end the greatest field 7.  If no
 * line stops, every id has exactly two distinct cluster ends, else TASKC_NOT_TWO_ENDS with stop_line 0 and stop_value the
 * lowest such id.  Output: ids ascending, cluster ends ascending within an id, "id \t end \t name \t strand \t start \t end
 * \n" with the integers in plain decimal.
 *
 * A stop ends the call as in the section above: it returns DSA_OK, the result names the lowest stopping line (1-based over
 * all pieces, or over the dedup text for TASKC_DEDUP), its bytes, the cause, its field and stop_value; a line's own stop beats
 * a run's on the same line; n_lines is that of the whole text and every other count is 0.  After a stop the ctx holds no
 * output of that kind, and the calls that need one return DSA_E_ARG.
 * One corner: the one-pass host tool reports a malformed field 0-2 on the line right behind a run before that run's missing
 * end; here the run in front of such a line is complete, and its missing end, on the lower line, is what is reported.  (A
 * line whose position field is malformed belongs to its run, so its own stop is never behind that run's.)
 * One ctx must not be used from two threads at once. */

#define TASKC_FEW_FIELDS    1
#define TASKC_BAD_INTEGER   2
#define TASKC_MISSING_END   3
#define TASKC_NOT_TWO_ENDS  4
#define TASKC_INPUT         0      /* source of taskc_regions: the text as added                                      */
#define TASKC_DEDUP         1      /* source: the output of the last taskc_dedup; taskc_fetch: that text              */
#define TASKC_REGIONS       2      /* taskc_fetch: the regions text of the last taskc_regions                         */

typedef struct taskc_result {
    int64_t n_lines;                   /* lines of the source text                                                     */
    int64_t n_runs;                    /* dedup: runs                                                                  */
    int64_t n_clusters;                /* regions: distinct ids                                                        */
    int64_t n_fragments;               /* dedup: fragments of all runs                                                 */
    int64_t n_kept_fragments;          /* dedup: fragments printed (two lines each)                                    */
    int64_t n_kept_runs;               /* dedup: runs that passed min_cluster_size                                     */
    int64_t out_bytes;                 /* bytes of the text made                                                       */
    int64_t stop_line;                 /* 1-based, 0: no stop or TASKC_NOT_TWO_ENDS                                    */
    int64_t stop_off, stop_len;        /* the stopping line is text[stop_off .. stop_off + stop_len) of the source     */
    int64_t stop_value;                /* TASKC_MISSING_END: the fragment; TASKC_NOT_TWO_ENDS: the id                  */
    int32_t stop_kind;                 /* TASKC_*, 0: no stop                                                          */
    int32_t stop_field;                /* the field that stopped, else -1                                              */
} taskc_result;

/* HIP-event times: upload and tables summed over the pieces since taskc_begin, the others of the most recent call. */
typedef struct taskc_timing {
    float   upload_ms;                 /* the pieces to the device (or the cover's output copied)                      */
    float   tables_ms;                 /* newline tables, line starts                                                  */
    float   parse_ms;                  /* the line rule, once per input                                                */
    float   sorts_ms;                  /* dedup: run heads, the sorts by (run, fragment) and (run, pos0, pos1)         */
    float   select_ms;                 /* dedup: winners, duplicates, counts per run, output lengths and offsets       */
    float   gather_ms;                 /* dedup: the kept lines copied                                                 */
    float   regions_ms;                /* regions: keys, sort, min / max / last per group, the ends of every id        */
    float   print_ms;                  /* regions: lengths, offsets, the text                                          */
    int64_t text_bytes;
    int64_t n_pieces;
} taskc_timing;

typedef struct taskc_ctx taskc_ctx;             /* opaque: the text, its lines and the two outputs     */

int taskc_create(int device, taskc_ctx** out);
void taskc_destroy(taskc_ctx* ctx);
/* Forgets the text and both outputs. */
int taskc_begin(taskc_ctx* ctx);
/* One piece from host memory.  final = 0: only whole lines are consumed (*consumed says how many bytes; give the rest again
 * in front of the next piece); final = 1: the piece's last line may lack its newline.  DSA_E_LIMIT for a piece of more than
 * 2^31 - 1 bytes or more than 2^31 - 1 lines in all.  Drops both outputs. */
int taskc_add(taskc_ctx* ctx, const uint8_t* text, int64_t len, int32_t final, int64_t* consumed);
/* The output of cover's last sct_cover as one piece, copied from device memory to device memory; cover may be reused or
 * destroyed afterwards.  DSA_E_ARG if it has no output or lives on another device. */
int taskc_add_cover(taskc_ctx* ctx, const sct_ctx* cover);
int taskc_dedup(taskc_ctx* ctx, int64_t min_cluster_size, taskc_result* result);
/* source: TASKC_INPUT or TASKC_DEDUP (DSA_E_ARG if there is no dedup text). */
int taskc_regions(taskc_ctx* ctx, int32_t source, taskc_result* result);
/* len bytes from offset of the dedup text (which = TASKC_DEDUP) or the regions text (TASKC_REGIONS) to the host. */
int taskc_fetch(taskc_ctx* ctx, int32_t which, int64_t offset, uint8_t* buf, int64_t len);
/* Everything taskt_parse_regions does, with the regions text of the last taskc_regions read where it lies: `into` (same
 * device, with an exon table) then holds the pairs for taskt_pairs_fetch and taskt_store_create.  Codes and the result are
 * taskt_parse_regions'. */
int taskc_parse_regions(taskc_ctx* ctx, taskt_ctx* into, const taskt_names* seq_names, taskt_result* result);
int taskc_get_timing(const taskc_ctx* ctx, taskc_timing* out);
const char* taskc_last_error(void);

/* ---- concordant clusters ------------------------------------------------------------------------------------------------
 * The concordant-cluster filter on cluster text in device memory (conc_*, defuse_amd/csrc/conc_api.hip).
 *
 * Between the set cover and the duplicate filter the pipeline drops every cluster whose two ends can be explained by one
 * locus (scripts/defuse_run.pl:484-505):
 *
 *     prep_local_alignment_seqs.pl -r FASTA -g GTF -c clusters.sc.unfilt -s 2000     > clusters.sc.local.seq
 *     localalign -m 10 -x -5 -g -5 -t 0.8                                            > clusters.sc.local.align
 *     cat clusters.sc.unfilt | filter_column.pl clusters.sc.local.align 0 1
 *
 * This section replaces the three steps in one call sequence over a taskc_ctx that holds clusters.sc.unfilt (taskc_add or
 * taskc_add_cover) and a task_reference that holds the FASTA; no sequence byte crosses the bus:
 *
 *     conc_models_create   once per run: the gene models, flattened by the host reader (defuse_amd/concfilter.py)
 *     conc_targets         every cluster end's targets: the genomic window, and one window per transcript of every
 *                          overlapping gene in whose coding sequence or UTR the genomic midpoint lies
 *     conc_align           SimpleAligner of every window against the other end's whole extent (la_api.hip's kernels)
 *     conc_filter          the clusters.sc.local.align text, and the cluster lines of the ids it does not name
 *     conc_into_taskc      that text into a taskc_ctx, device to device: taskc_dedup follows
 *
 * Canonical order.  Perl prints clusters, genes and transcripts in hash order.  Here targets (and so the local.align lines)
 * come by cluster id ascending, end 0 then 1, the genomic target first, then genes ascending by id bytes, then a gene's
 * transcripts ascending by name bytes.  The filtered text is in file order, as filter_column.pl's.
 *
 * Positions are kept doubled ("half-units"), since (start + end) / 2 may end in .5; every test is on integers.
 * Bio::DB::Fasta::subseq and caloffset are restated literally: `start ||= 1`, `stop ||= length`, the swap with reverse and
 * complement when start > stop, each bound minus 1 clamped to [0, L - 1] and truncated.  A window is clipped, not padded.
 *
 * Where this section stops and the scripts do not (conc_result.stop_kind; nothing is output on a stop):
 *   - a line with fewer than eight fields or with a field 0, 1, 6 or 7 that taskc_regions does not read as an integer
 *     (CONC_FEW_FIELDS, CONC_BAD_INTEGER, the line in stop_line): Perl takes any text as a key and numifies the coordinates,
 *     and filter_column.pl dies only on a line without field 0;
 *   - a cluster id whose ends are not exactly 0 and 1 (CONC_NOT_TWO_ENDS, the id in stop_value): Perl dies on a missing end
 *     0 or 1 and ignores ends with other numbers;
 *   - a strand that is neither "+" nor "-" (CONC_BAD_STRAND): Perl treats it as a minus strand that equals no transcript's;
 *   - an empty reference name (CONC_EMPTY_NAME): Perl dies in the bins of the null transcript's chromosome;
 *   - an other end whose name the FASTA lacks (CONC_NO_OTHER_SEQ): Perl dies at the first target of that end that prints,
 *     and not at all if none does;
 *   - an other end on a sequence without bytes (CONC_EMPTY_OTHER): the maximum score is 0 and localalign prints "-nan".
 * DSA_E_LIMIT: a name of the form `name:a-b` (subseq would cut it), a coordinate beyond +-TASK_MAX_COORD, a range outside
 * [0, TASK_MAX_PARAM], a target on a sequence without bytes, more than 2^31 - 1 targets.  A stop is reported first.
 *
 * Host round trips: the counts that size a buffer (targets, kept targets, bytes of either text, the first stop) and, in
 * conc_align, one 32-byte pair per target down (the wave planner of la_api.hip reads the lengths) and up again with the
 * lanes and waves it plans.  Scores stay on the device.
 *
 * Out of scope: select_fusion_clusters.pl (its nearest gene among equally near ones is Perl's hash order, so its output is
 * no function of its input); a defuse_glue step and a C++ GTF reader (the tools keep their paths); the
 * clusters.sc.local.seq text itself (the descriptors stand for it); more than one GPU.  There is no CPU path.
 */
#define CONC_FEW_FIELDS     1      /* = TASKC_FEW_FIELDS                                                            */
#define CONC_BAD_INTEGER    2      /* = TASKC_BAD_INTEGER                                                           */
#define CONC_NOT_TWO_ENDS   3
#define CONC_BAD_STRAND     4
#define CONC_EMPTY_NAME     5
#define CONC_NO_OTHER_SEQ   6
#define CONC_EMPTY_OTHER    7

#define CONC_ALIGN_TEXT     0      /* conc_fetch: clusters.sc.local.align                                           */
#define CONC_FILTERED       1      /* conc_fetch: the cluster lines that stay                                       */

#define CONC_KIND_GENOMIC     0
#define CONC_KIND_TRANSCRIPT  1

typedef struct conc_gene {
    int32_t start, end;             /* the region: [least first-exon start, greatest last-sorted-exon end]           */
    int32_t tx_first, tx_count;     /* its transcripts: gene_tx[tx_first ..), ascending by name bytes                */
} conc_gene;

typedef struct conc_transcript {
    int32_t gene, chrom;
    int32_t strand;                 /* 0 "+", 1 "-", 2 anything else                                                 */
    int32_t exon_first, exon_count; /* exons[..], stably sorted by start                                             */
    int32_t expr_first, expr_count; /* expressed[..]: CDS, 5' UTR and 3' UTR pieces                                  */
    int32_t pad_;
} conc_transcript;

typedef struct conc_interval {
    int32_t start, end;
} conc_interval;

typedef struct conc_name {
    int64_t off;                    /* names[off .. off + len)                                                       */
    int32_t len;
    int32_t pad_;
} conc_name;

/* Host arrays, copied by conc_models_create.  Genes are numbered ascending by id bytes; chrom_names and transcript_names
 * ascend strictly by their bytes; chrom_genes[chrom_gene_first[c] .. chrom_gene_first[c + 1]) are the genes an accepted
 * line put on chromosome c, ascending by region start; seq_names[k] names sequence k of the task_reference. */
typedef struct conc_models_desc {
    const conc_gene*       genes;
    const int32_t*         gene_tx;
    const conc_transcript* transcripts;
    const conc_interval*   exons;
    const conc_interval*   expressed;
    const int32_t*         chrom_gene_first;   /* n_chroms + 1 */
    const int32_t*         chrom_genes;
    const uint8_t*         names;
    const conc_name*       chrom_names;
    const conc_name*       transcript_names;
    const conc_name*       seq_names;
    int64_t n_genes, n_gene_tx, n_transcripts, n_exons, n_expressed, n_chrom_genes, names_len, n_chroms, n_seqs;
} conc_models_desc;

/* One line of clusters.sc.local.seq: field 1 is sequence `seq` [start, start + len), reversed and complemented where revcomp
 * is set; field 2 is sequence other_seq [other_start, + other_len), likewise by other_rev.  0-based, clipped. */
typedef struct conc_target {
    int32_t cluster_id, cluster_end;
    int32_t kind;                   /* CONC_KIND_*                                                                   */
    int32_t name;                   /* transcript index; genomic: chromosome index, -1 for a name the models lack    */
    int32_t seq, start, len, revcomp;
    int32_t other_seq, other_start, other_len, other_rev;
} conc_target;

typedef struct conc_result {
    int64_t n_lines;                /* cluster lines read                                                            */
    int64_t n_clusters;
    int64_t n_targets;
    int64_t n_kept_targets;         /* conc_filter: lines of the local.align text                                    */
    int64_t align_bytes;
    int64_t n_hit_clusters;         /* ids the local.align text names                                                */
    int64_t n_kept_lines;
    int64_t out_bytes;
    int64_t n_noncanonical;         /* cluster lines whose id text is not the plain decimal of its value ("007", "+7"):
                                       Perl's string keys tell such ids apart, this section compares values          */
    int64_t stop_line;              /* 1-based, 0 where the stop is not at a line                                    */
    int64_t stop_value;             /* the cluster id of a stop at a cluster                                         */
    int32_t stop_kind;              /* 0 or CONC_*                                                                   */
    int32_t stop_field;             /* -1 or the field of a CONC_BAD_INTEGER                                         */
} conc_result;

/* HIP-event times of the last call of each stage. */
typedef struct conc_timing {
    float   targets_ms;             /* groups (taskc_regions), count, scan, emit                                     */
    float   sort_ms;                /* canonical order                                                               */
    float   download_ms;            /* the descriptors to the wave planner                                           */
    float   pack_ms;                /* k_pack_pairs                                                                  */
    float   dp_ms;                  /* k_la16 / k_la32                                                               */
    float   print_ms;               /* decide, lengths, scan, the local.align text                                   */
    float   filter_ms;              /* hit ids, line lengths, scan, gather                                           */
    float   pad_;
    int64_t cells;
    int64_t n_packed16, n_int32;
} conc_timing;

typedef struct conc_models conc_models;
typedef struct conc_ctx conc_ctx;

/* DSA_E_ARG, before a device is touched, for an index outside its table, name tables that do not ascend, a negative count;
 * DSA_E_LIMIT for a `name:a-b` name or a coordinate beyond +-TASK_MAX_COORD. */
int conc_models_create(int device, const conc_models_desc* desc, conc_models** out);
void conc_models_destroy(conc_models* models);

int conc_create(int device, conc_ctx** out);
void conc_destroy(conc_ctx* ctx);

/* The targets of the input text of `clusters`, whose groups by (id, end) it makes with taskc_regions(TASKC_INPUT): the
 * regions text of `clusters` is that one afterwards.  reference must have models' n_seqs sequences.  The ctx reads the
 * text of `clusters` in place until conc_filter has run: no other call on `clusters` in between. */
int conc_targets(conc_ctx* ctx, taskc_ctx* clusters, const conc_models* models, const task_reference* reference, int32_t range,
                 conc_result* result);
int conc_fetch_targets(conc_ctx* ctx, conc_target* out, int64_t n);

/* Scores of all targets.  match > 0; min_score of a pair is threshold_min_score(score_max(other_len, match), threshold), as
 * bin/localalign derives it: a score below it is not exact.  DSA_E_ARG without targets of conc_targets. */
int conc_align(conc_ctx* ctx, const task_reference* reference, int32_t match, int32_t mismatch, int32_t gap, double threshold,
               conc_result* result);
int conc_fetch_scores(conc_ctx* ctx, int32_t* out, int64_t n);

/* Both texts, with the scores and the threshold of conc_align. */
int conc_filter(conc_ctx* ctx, conc_result* result);
int conc_fetch(conc_ctx* ctx, int32_t which, int64_t offset, uint8_t* buf, int64_t len);

int conc_get_timing(const conc_ctx* ctx, conc_timing* out);
const char* conc_last_error(void);

/* The filtered text behind the text of `into` (another taskc_ctx than the one conc_targets read, or that one after
 * taskc_begin), as taskc_add_cover does with a cover's output.  It is a conc_ function with the conc_ctx first, not a
 * taskc_add_*: conc_api.hip implements it and its errors are conc_last_error()'s, and every taskc_* function of this header
 * is bound by one module (defuse_amd/clusterregions.py) whose table the ABI check counts. */
int conc_into_taskc(const conc_ctx* ctx, taskc_ctx* into);

#ifdef __cplusplus
}
#endif
#endif
