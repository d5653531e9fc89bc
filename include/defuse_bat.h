/*
 * defuse_bat.h — C ABI of the MI355X batch assembly between the candidate loop and the split-read DP ("bat").
 *
 * Replaces, for a whole batch of kept candidates at once, what SplitReadRealigner::DoAlignment does per candidate before
 * it calls SplitAlignmentTask::Align:
 *
 *     SplitReadRealigner::AddReads   tools/SplitAlignment.cpp:253-264   -> bat_reads_create
 *     mAlignTasks                    tools/SplitAlignment.cpp:294       -> bat_windows_create
 *     mReads[readID.id]              tools/SplitAlignment.cpp:286       -> bat_assemble, the lookup
 *     ReverseComplement              tools/SplitAlignment.cpp:287-290, tools/Common.cpp:32-54   -> bat_assemble, the gather
 *
 * The result is a batch in the form of defuse_dsa.h (ref_bytes, dsa_fusion[], read_bytes, dsa_pair[]) that never leaves
 * the device: bat_batch_view hands its four device pointers to dsa_upload_device.  With cand_enumerate_device in front
 * and dsa_copy_records_device + eval_groups_device behind, alignments go up and groups and kept records come down.
 *
 * The batch, exactly:
 *   pairs[k] belongs to cands[k]: frag, read_end and revcomp are copied, pad_ is zero; read_len is the length of the read
 *     with the key ReadID.id = (fragment, read_end) — 0 if no such read was given — and read_off the sum of the lengths
 *     before it.
 *   read_bytes is the concatenation of those reads; where revcomp is set the read is reversed and A<->T, C<->G, a<->t,
 *     c<->g are exchanged.  Every other byte value stays as it is.
 *   A fusion enters fusions[] when its first candidate is met, whatever the order of the candidates; ref_bytes is window 0
 *     then window 1 of each such fusion, in that order.  Candidates are not de-duplicated here.
 *
 * Plain C types; host pointers unless the name says _device.  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: creating an object fails with DSA_E_DEVICE without a GPU.  Argument errors that can
 * be told from the arguments alone are found before a device is touched.  One object must not be used from two threads at
 * once.  Out of scope: more than one GPU per chain, and reads or windows beyond the range of the 16-bit DP kernels
 * (dsa_upload_device refuses those; such a batch is fetched and goes through dsa_upload).
 */
#ifndef DEFUSE_BAT_H_
#define DEFUSE_BAT_H_

#include <stdint.h>

#include "defuse_cand.h"
#include "defuse_dsa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One read of the run: bytes[off .. off + len) under the key ReadID.id (tools/Common.h: fragment in bits 0-30, read end
 * in bit 31). */
typedef struct bat_read {
    int64_t off;                       /* into the bytes given to bat_reads_create                                 */
    int32_t len;                       /* >= 0                                                                     */
    int32_t fragment;                  /* ReadID.fragmentIndex, in [0, 2^31)                                       */
    int32_t read_end;                  /* 0 / 1                                                                    */
    int32_t pad_;
} bat_read;

/* The assembled batch on the device; the arguments of dsa_upload_device in its order.  Valid until the next
 * bat_assemble* on the batch or its destruction. */
typedef struct bat_view {
    const void* ref_bytes;             /* device pointers; never NULL after a successful assembly                  */
    const void* fusions;               /* dsa_fusion[n_fusions]                                                    */
    const void* read_bytes;
    const void* pairs;                 /* dsa_pair[n_pairs]                                                        */
    int64_t ref_bytes_len;
    int64_t read_bytes_len;
    int64_t n_pairs;
    int32_t n_fusions;
    int32_t device;
} bat_view;

/* HIP-event times of the most recent bat_assemble* of a batch. */
typedef struct bat_timing {
    float   upload_ms;                 /* candidates to the device (bat_assemble only)                             */
    float   lookup_ms;                 /* read and window slot of every candidate, first position per window       */
    float   scan_ms;                   /* sums, compaction, sort of the used fusions, descriptors                  */
    float   gather_ms;                 /* the two gather launches: reads, then windows                             */
    int64_t n_candidates;
    int64_t n_fusions;
    int64_t read_bytes;                /* bytes the gathers wrote (they read as many)                              */
    int64_t ref_bytes;
} bat_timing;

typedef struct bat_reads bat_reads;         /* opaque: the reads of a run on one device                          */
typedef struct bat_windows bat_windows;     /* opaque: both windows of every task on one device                  */
typedef struct bat_batch bat_batch;         /* opaque: the buffers of an assembled batch, reused call after call */

/* AddReads for reads[0..n): of several reads with one key the LAST given wins (mReads[id] = seq); a key that was never
 * given reads as the empty string.  DSA_E_ARG, naming the record, for a fragment outside [0, 2^31), a read_end other than
 * 0 / 1, a negative len, or off / len outside bytes.  n = 0 is allowed (every lookup is empty).  n > 2^31 - 1 is
 * DSA_E_LIMIT.  The bytes are copied: the caller's buffers are free on return. */
int bat_reads_create(int device, const uint8_t* bytes, int64_t bytes_len, const bat_read* reads, int64_t n, bat_reads** out);
void bat_reads_destroy(bat_reads* reads);

/* mAlignTasks: fusions[k] gives the two windows of task fusion_id as offsets into ref_bytes, checked as dsa_upload checks
 * them (DSA_E_ARG for a window outside ref_bytes, DSA_E_LIMIT for one longer than dsa_limits.max_ref_len).  Two entries
 * with one fusion_id are DSA_E_ARG.  ref_bytes_len > 2^31 - 1 is DSA_E_LIMIT (the offsets are int32). */
int bat_windows_create(int device, const uint8_t* ref_bytes, int64_t ref_bytes_len, const dsa_fusion* fusions, int32_t n, bat_windows** out);
void bat_windows_destroy(bat_windows* windows);

int bat_batch_create(int device, bat_batch** out);
void bat_batch_destroy(bat_batch* batch);

/* The batch of cands[0..n) (see the top of this header) into the buffers of `batch`, which grow as needed and are kept.
 * DSA_E_ARG: an object is missing, the three objects are not on one device, or a fusion_id that `windows` does not have —
 * the message names the lowest such record index.  DSA_E_LIMIT: n > 2^31 - 1, or a read_bytes or ref_bytes total above
 * 2^31 - 1 (the offsets of dsa_pair and dsa_fusion are int32); the totals are formed in 64 bits and tested before anything
 * of that size is allocated.  n = 0 gives an empty batch.  After a failure the batch is empty.
 * bat_assemble_device takes the records from device memory of the same GPU (cand_records_device); they must be complete
 * (the call that made them has returned) and stay untouched until the call returns. */
int bat_assemble(bat_reads* reads, bat_windows* windows, const cand_record* cands, int64_t n, bat_batch* batch);
int bat_assemble_device(bat_reads* reads, bat_windows* windows, const void* cands_device, int64_t n, bat_batch* batch);

int bat_batch_view(const bat_batch* batch, bat_view* out);
/* Downloads the four arrays (any buffer whose capacity is 0 may be NULL).  DSA_E_CAPACITY if one of them does not fit;
 * nothing is written then.  Capacities are in elements: bytes, dsa_fusion, bytes, dsa_pair. */
int bat_batch_fetch(bat_batch* batch, uint8_t* ref_bytes, int64_t ref_cap, dsa_fusion* fusions, int64_t fusions_cap,
                    uint8_t* read_bytes, int64_t read_cap, dsa_pair* pairs, int64_t pairs_cap);
int bat_get_timing(const bat_batch* batch, bat_timing* out);

const char* bat_last_error(void);

/* ---- the candidates of a session, left on the device (the session and its rules: defuse_cand.h) -------------------- */
/* cand_enumerate with the records left in the session's device buffer: the same rules and the same commit of the seen
 * keys, but no capacity protocol and no download (timing->download_ms is 0); *n_out receives their number.
 * cand_records_device gives the device pointer and the count of the records of the latest cand_enumerate_device of the
 * session (NULL and 0 after any other call on it, a failed one included).  They are complete when the call returns and
 * valid until the next call on that session; bat_assemble_device takes them from there. */
int cand_enumerate_device(cand_session* session, const cand_alignment* alignments, int64_t n, int32_t order, int64_t* n_out,
                          cand_timing* timing);
int cand_records_device(const cand_session* session, const void** dev, int64_t* n);

#ifdef __cplusplus
}
#endif
#endif
