/*
 * defuse_eval.h — C ABI of the MI355X evaluation of split alignments: per fusion, the best supported breakpoint.
 *
 * Replaces the arithmetic of SplitAlignmentTask::Evaluate (tools/SplitAlignment.cpp:484-594) for all groups of a batch at
 * once; the sequence assembly and the three writers (:596-624) stay with the caller, who has the tasks.
 *
 * Input: n records (dsa_record of defuse_dsa.h, 40 bytes), of which only fusion_id, ref_first, ref_second, read_first,
 * read_second and score are read.  Negative coordinates and negative scores are valid: the tool reads them from a text file.
 *
 * Groups: a group is a maximal run of consecutive records with equal fusion_id, exactly as ReadSortedAlignments forms
 * them (tools/SplitAlignment.cpp:319-369).  A fusion id that comes back later opens a new group; nothing is sorted by id and
 * nothing requires sorted ids.
 *
 * Per group (:496-520): the scores of the records are summed per refSplit = (ref_first, ref_second); the best split is the one
 * with the largest sum, ties going to the lexicographically smallest (first, second) compared as signed ints — the
 * reference walks a std::map in ascending key order with a strict '>' from maxScore = -1 (canonical order of SURVEY 8(c)).
 * If no split has a sum greater than -1 the group has no best split (EVAL_NO_SPLIT: the reference's "Unable to find max score
 * split").  Sums are accumulated in 64 bits; if the sum of ANY split of any group leaves the int32 range the call fails with
 * DSA_E_LIMIT, because the reference's int would overflow there.
 *
 * Kept records: the records of a group at its best split (:522-530).  The kept list holds their indices into the input,
 * group after group, in input order within a group: the order WriteAlignments writes them in (:617-624).
 *
 * Statistics (:571-587), over the kept records of a group SERIALLY IN RECORD ORDER, starting from 0.0:
 *     posRange = (double)(left + right - 8)            posValue = max(0, left - 4)
 *     minRange = floor(0.5 * (left + right - 8))       minValue = max(0, min(left - 4, right - 4))
 *     pos_sum += posValue / posRange                   min_sum += minValue / minRange
 * with left = read_first, right = read_second; every term is an IEEE double division and every addition an IEEE double
 * addition in that order (no reassociation, no tree), so the sums equal the reference's bit for bit.  left + right is formed
 * in 64 bits.  A kept record with left + right - 8 <= 1 has posRange or minRange 0 or below: a division by zero gives a NaN
 * whose sign differs between x86 and the GPU (and "%g" prints it), so such a group is only flagged (EVAL_HOST_STATS), its
 * pos_sum / min_sum are left unspecified and the caller computes them itself.  A record of that kind that is not kept does
 * not flag its group.
 *
 * Plain C types; host pointers unless the name says "_device".  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: without a GPU eval_create returns DSA_E_DEVICE.  A ctx is bound to one device and
 * must not be used from two threads at once.
 */
#ifndef DEFUSE_EVAL_H_
#define DEFUSE_EVAL_H_

#include <stdint.h>

#include "defuse_dsa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EVAL_NO_SPLIT    1   /* no split with a sum > -1: only fusion_id, first_record and n_records are meaningful */
#define EVAL_HOST_STATS  2   /* a kept record has read_first + read_second - 8 <= 1: pos_sum / min_sum are the caller's */

typedef struct eval_group {
    int32_t fusion_id;
    int32_t status;            /* EVAL_* bits                                                  */
    int64_t first_record;      /* the group is records [first_record, first_record + n_records) */
    int64_t n_records;
    int32_t best_first;        /* the best refSplit                                            */
    int32_t best_second;
    int32_t best_score;        /* its summed score                                             */
    int32_t pad_;
    int64_t count;             /* records at the best split = the group's kept records         */
    int64_t kept_off;          /* they are kept[kept_off .. kept_off + count)                  */
    double  pos_sum;           /* the caller divides by count (:586-587)                       */
    double  min_sum;
} eval_group;

typedef struct eval_timing {   /* of the most recent eval_groups / eval_groups_device (HIP events) */
    float   upload_ms;         /* records host -> device (0 for eval_groups_device)            */
    float   device_ms;         /* all kernels                                                  */
    float   download_ms;       /* groups and kept list device -> host                          */
    float   pad_;
    int64_t n_records;
    int64_t n_groups;
    int64_t n_runs;            /* distinct (group, split) pairs                                */
    int64_t n_kept;
    int64_t n_flagged;         /* groups with EVAL_HOST_STATS                                  */
} eval_timing;

typedef struct eval_ctx eval_ctx;   /* opaque: the device buffers of one caller on one device, kept between calls */

int  eval_create(int device, eval_ctx** out);
void eval_destroy(eval_ctx* ctx);
/* Evaluates the n records (n may be 0: zero groups).  *n_groups and *n_kept always receive the counts.  If they exceed
 * group_cap or kept_cap the call returns DSA_E_CAPACITY and writes nothing else (groups and kept may then be NULL); a second
 * call with room for them succeeds.  DSA_E_LIMIT: a split's sum left the int32 range, or n >= 2^31 - 2. */
int  eval_groups(eval_ctx* ctx, const dsa_record* records, int64_t n,
                 eval_group* groups, int64_t group_cap, int64_t* n_groups,
                 int64_t* kept, int64_t kept_cap, int64_t* n_kept);
/* The same on records that are already in memory of the ctx's device, e.g. what dsa_copy_records_device filled: they are
 * read in place and never visit the host.  groups and kept are host pointers as above.  records_device must be aligned to
 * 8 bytes (any hipMalloc result is), and whatever wrote the records must have COMPLETED before the call: the ctx reads them
 * on a non-blocking stream of its own, which waits for no other stream, the null stream included.  dsa_copy_records_device
 * returns after its copy is done; a caller whose own kernel produced the records synchronises that stream first. */
int  eval_groups_device(eval_ctx* ctx, const void* records_device, int64_t n,
                        eval_group* groups, int64_t group_cap, int64_t* n_groups,
                        int64_t* kept, int64_t kept_cap, int64_t* n_kept);
int  eval_get_timing(const eval_ctx* ctx, eval_timing* out);
const char* eval_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
