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
 * Strings stay with the caller, who resolves every name to a dense index once: sequences of the FASTA (task_seq), chromosomes
 * and transcripts of the exon table, and the reference numbering of cand_region.ref.
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
 * cand_table_create from device regions, reading FASTA / .fai / exon text, more than one GPU per chain.
 */
#ifndef DEFUSE_TASK_H_
#define DEFUSE_TASK_H_

#include <stdint.h>

#include "defuse_bat.h"
#include "defuse_cand.h"
#include "defuse_dsa.h"
#include "defuse_pred.h"

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

#ifdef __cplusplus
}
#endif
#endif
