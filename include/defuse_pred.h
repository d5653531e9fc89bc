/*
 * defuse_pred.h — C ABI of the MI355X prediction of each fusion's sequence and break positions ("pred").
 *
 * Replaces, for all groups of a batch at once, the rest of SplitAlignmentTask::Evaluate after the best split is known:
 *
 *     the sequence assembly      tools/SplitAlignment.cpp:545-551   -> pred_predict*, the gather
 *     the two break positions    tools/SplitAlignment.cpp:553-569   -> pred_predict*, the plan
 *     the two averages           tools/SplitAlignment.cpp:589-591   -> pred_predict*, the plan
 *
 * It follows eval in the resident chain (cand_enumerate_device, bat_assemble_device, dsa_upload_device / dsa_run,
 * dsa_copy_records_device, eval_groups_device): the windows that bat_windows_create put on the device are read in place, so
 * a caller of the chain keeps no host copy of them, and what comes down is what WriteSequence and WriteBreak print.
 *
 * Per group, with (first, second) = the group's best split (eval_group.best_first / best_second), seq0 / seq1 the task's two
 * windows of seq_len[0] / seq_len[1] bytes and rem0 / rem1 its two remainder sequences:
 *     sequence     = rem0 + seq0[0 : first) + '|' + seq1[second + 1 : ) + rem1
 *     break_pos[0] = seq_start[0] + first - 1            on the plus strand,  seq_start[0] + seq_len[0] - first       on minus
 *     break_pos[1] = seq_start[1] + second + 1           on the plus strand,  seq_start[1] + seq_len[1] - second - 2  on minus
 *     pos_avg      = pos_sum / (double)count             min_avg = min_sum / (double)count
 * each average one IEEE double division, bit-equal to the host's.  The sequences lie in seq_bytes one after the other in
 * group order, without padding or terminator; seq_off is the 64-bit running sum of the lengths, so the total may pass 2^31.
 *
 * A group gets seq_len = 0, and only its fusion_id, status and count are meaningful (the other fields are zero), if
 *   - it carries EVAL_NO_SPLIT, or
 *   - its fusion_id has no task (PRED_NO_TASK; the reference would evaluate a default-constructed task there), or
 *   - its split fails one of the reference's two DebugChecks (PRED_OUT_OF_WINDOW): first < 0, first > seq_len[0],
 *     second + 1 < 0 or second + 1 >= seq_len[1].  Negative coordinates are legal input, as they are for eval_groups.
 * PRED_OUT_OF_WINDOW is only tested where there is a task and a split.  A group with EVAL_HOST_STATS gets its sequence and
 * break positions; its two averages are left unspecified, as its sums already are.
 *
 * eval_ctx and its groups.  pred_predict_resident reads the groups from the device buffer of an eval_ctx, which therefore
 * KEEPS THE GROUPS OF ITS LATEST SUCCESSFUL eval_groups / eval_groups_device CALL ON THE DEVICE UNTIL THE NEXT CALL ON IT.
 * A call that failed, or that was refused for capacity, leaves the ctx without such groups.
 *
 * Plain C types; host pointers unless the name says _device.  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: creating an object fails with DSA_E_DEVICE without a GPU.  Argument errors that can
 * be told from the arguments alone are found before a device is touched.  One object must not be used from two threads at
 * once.  Out of scope: the tools (they keep their host evaluators), more than one GPU per chain, a streamed entry.  The
 * two texts themselves are printed on the device by defuse_ptext.h.
 */
#ifndef DEFUSE_PRED_H_
#define DEFUSE_PRED_H_

#include <stdint.h>

#include "defuse_bat.h"
#include "defuse_dsa.h"
#include "defuse_eval.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PRED_NO_TASK        4   /* or-ed into the group's EVAL_* bits: no task has the group's fusion_id               */
#define PRED_OUT_OF_WINDOW  8   /* the best split lies outside the task's windows                                      */

/* One SplitAlignmentTask, as far as Evaluate reads it; index 0 / 1 is the cluster end. */
typedef struct pred_task {
    int32_t fusion_id;
    int32_t pad_;
    int32_t seq_start[2];              /* mSplitAlignSeqStart, as FastaIndex::Get left it after clipping               */
    int32_t seq_len[2];                /* mSplitAlignSeqLength, likewise: the length of the window in `windows`; below */
                                       /* 0, as Get leaves a length it was asked with below 0: the window is empty     */
    int32_t seq_strand[2];             /* mSplitSeqStrand: 0 = PlusStrand, 1 = MinusStrand                             */
    int32_t rem_len[2];                /* mSplitRemainderSeq is rem_bytes[rem_off .. rem_off + rem_len)                */
    int64_t rem_off[2];
} pred_task;

typedef struct pred_result {
    int32_t fusion_id;                 /* the group's fusion                                                           */
    int32_t status;                    /* the group's EVAL_* bits, or-ed with PRED_*                                   */
    int64_t seq_off;                   /* the sequence is seq_bytes[seq_off .. seq_off + seq_len)                      */
    int32_t seq_len;                   /* including the '|' separator; 0: see the top of this header                   */
    int32_t break_pos[2];
    int32_t pad_;
    int64_t count;                     /* the group's count                                                            */
    double  pos_avg;
    double  min_avg;
} pred_result;

/* The results of the latest pred_predict* of a ctx on the device.  Valid until the next pred_predict* on the ctx or its
 * destruction. */
typedef struct pred_device_view {
    const void* results;               /* pred_result[n_results]; device pointers, never NULL after a successful call  */
    const void* seq_bytes;
    int64_t n_results;
    int64_t seq_bytes_len;
    int32_t device;
    int32_t pad_;
} pred_device_view;

/* HIP-event times of the most recent pred_predict* of a ctx, and of the most recent pred_fetch after it. */
typedef struct pred_timing {
    float   upload_ms;                 /* groups to the device (pred_predict only)                                     */
    float   plan_ms;                   /* task lookup, checks, lengths, break positions, averages                      */
    float   scan_ms;                   /* the 64-bit sum of the lengths, its total to the host, the descriptors        */
    float   gather_ms;                 /* the two gather launches: remainders, then windows                            */
    float   download_ms;               /* pred_fetch                                                                   */
    float   pad_;
    int64_t n_groups;
    int64_t seq_bytes;                 /* bytes the gathers and the separators wrote                                   */
} pred_timing;

typedef struct pred_tasks pred_tasks;       /* opaque: the tasks of a run on one device                          */
typedef struct pred_ctx pred_ctx;           /* opaque: the output buffers of one caller, reused call after call  */

/* The tasks of a run.  `windows` is on the same device and has both windows of every task; they are read in place, no second
 * copy is made, and the caller keeps `windows` alive as long as the store.  rem_bytes is copied: the caller's buffers are
 * free on return.  DSA_E_ARG, naming the record, for a strand other than 0 / 1, a negative remainder length, a remainder
 * outside rem_bytes, two tasks with one fusion_id, a fusion_id that `windows` does not have, or a seq_len that is not the
 * length of its window (max(seq_len, 0): a negative mSplitAlignSeqLength goes with an empty window, the DebugChecks see the
 * empty string, and the break positions are formed from the negative number, as the reference forms them).  DSA_E_LIMIT for a task whose longest sequence would pass 2^31 - 1 bytes.  n = 0 is allowed. */
int pred_tasks_create(int device, const bat_windows* windows, const uint8_t* rem_bytes, int64_t rem_bytes_len,
                      const pred_task* tasks, int64_t n, pred_tasks** out);
void pred_tasks_destroy(pred_tasks* tasks);

int pred_create(int device, pred_ctx** out);
void pred_destroy(pred_ctx* ctx);

/* One pred_result per group, in group order, and the sequences, left on the device in the buffers of `ctx`, which grow as
 * needed and are kept.  groups[0 .. n_groups) is what eval_groups* returned.  n_groups = 0 gives empty results.  After a
 * failure the results are empty.  DSA_E_ARG: an object is missing or the objects are not on one device; DSA_E_LIMIT:
 * n_groups > 2^30 - 1. */
int pred_predict(pred_ctx* ctx, const pred_tasks* tasks, const eval_group* groups, int64_t n_groups);
/* The same on the groups in the device buffer of `eval` (see the top of this header): they never visit the host.
 * DSA_E_ARG if that ctx has no completed evaluation, or if its latest call failed or was refused for capacity. */
int pred_predict_resident(pred_ctx* ctx, const pred_tasks* tasks, const eval_ctx* eval);

int pred_view(const pred_ctx* ctx, pred_device_view* out);
/* Downloads the results and the sequences (a buffer whose capacity is 0 may be NULL).  DSA_E_CAPACITY if either does not
 * fit; nothing is written then.  Capacities are in elements: pred_result, bytes. */
int pred_fetch(pred_ctx* ctx, pred_result* results, int64_t results_cap, uint8_t* seq_bytes, int64_t seq_cap);
int pred_get_timing(const pred_ctx* ctx, pred_timing* out);

const char* pred_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
