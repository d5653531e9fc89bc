/*
 * defuse_rec.h — C ABI of the MI355X record store: the split-alignment records of any number of batches, brought into the
 * order the pipeline's sort gives their lines, and printed.
 *
 * Between alignment and evaluation the reference runs `sort -n -k 1` per chunk and `sort -m -n -k 1` over the chunks
 * (scripts/defuse_run.pl:528,533), and evalsplitalign forms its groups from runs of equal fusion id in that file
 * (defuse_eval.h).  A store takes the records of all batches of a run (dsa_record of defuse_dsa.h, 40 bytes), sorts them on
 * the device into that file's order and prints its lines, so that eval_groups_device sees the groups and the record order
 * evalsplitalign would see without a record visiting the host unprinted.
 *
 * The line of a record is SplitAlignment::WriteAlignment: the nine fields fusion_id, frag, read_end, revcomp, ref_first,
 * ref_second, read_first, read_second, score, each as "%d" followed by a tab, then '\n'.  pair_idx is not printed and takes
 * no part in the order.
 *
 * The order is that of LC_ALL=C sort -n -k 1 on those lines, stated two equivalent ways:
 *   1. ascending by the numeric value of fusion_id, then ascending by the bytes of the whole line;
 *   2. ascending by fusion_id, then lexicographically by a per-field key of fields 2-9: the "%d" text and its tab read as up
 *      to 12 symbols of base 12, left-aligned and padded with 0, where tab is 0, '-' is 1 and the digits are 2..11
 *      (12^12 < 2^44).
 * Byte order is not numeric order: 100 sorts before 99, -1 before -10 before -9, and every negative value before every
 * non-negative one.  Records equal in all nine fields keep the order they were appended in (the sort is stable).  Only the C
 * locale's order is built.
 *
 * Plain C types; host pointers unless the name says "_device".  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: without a GPU rec_create returns DSA_E_DEVICE.  A store is bound to one device and
 * must not be used from two threads at once.  Every call returns after its device work is done.
 */
#ifndef DEFUSE_REC_H_
#define DEFUSE_REC_H_

#include <stdint.h>

#include "defuse_dsa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rec_timing {    /* HIP events                                                                          */
    float   append_ms;         /* all copies into the store since rec_create / rec_clear, growth included             */
    float   keys_ms;           /* of the most recent rec_sort: the key kernel                                         */
    float   sort_ms;           /*   the radix sorts and the key gathers between them                                  */
    float   gather_ms;         /*   the permutation of the records                                                    */
    float   format_ms;         /* of the most recent rec_text: lengths, scan and the write kernel                     */
    float   write_ms;          /*   of which the write kernel                                                         */
    float   download_ms;       /* of the most recent rec_text or rec_download: device -> host                         */
    float   pad_;
    int64_t n_records;         /* in the store                                                                        */
    int64_t n_sorts;           /* radix sorts of the most recent rec_sort: 7, or 9 with read_end / revcomp beyond 0/1 */
    int64_t text_bytes;        /* of the most recent rec_text                                                         */
} rec_timing;

typedef struct rec_store rec_store;   /* opaque: the records of one run on one device */

int  rec_create(int device, rec_store** out);
void rec_destroy(rec_store* s);
/* Empties the store; the device buffers stay. */
int  rec_clear(rec_store* s);
/* Adds n records behind the store's last one.  Growing keeps what the store holds.  DSA_E_LIMIT: the store would hold
 * 2^31 - 2 records or more (the bound of eval_groups).  Any append, rec_sort and rec_clear invalidate the pointers
 * rec_tail and rec_records_device gave out. */
int  rec_append(rec_store* s, const dsa_record* records, int64_t n);
/* The same for records in memory of the store's device; whatever wrote them must have completed. */
int  rec_append_device(rec_store* s, const void* records_device, int64_t n);
/* Zero-copy hand-over, e.g. from dsa_copy_records_device: *tail_device receives room for `room` records behind the store's
 * last one, and rec_commit(n) adds the first n <= room of them once their producer has completed.  A new rec_tail
 * invalidates the previous pointer.  rec_commit without a preceding rec_tail, a second rec_commit on one rec_tail, or
 * n > room is DSA_E_ARG. */
int  rec_tail(rec_store* s, int64_t room, void** tail_device);
int  rec_commit(rec_store* s, int64_t n);
/* Brings the records into the order above.  0 or 1 record is fine; a second rec_sort changes nothing; appending after a
 * sort and sorting again gives the array one sort of everything gives. */
int  rec_sort(rec_store* s);
int  rec_count(const rec_store* s, int64_t* n);
/* The store's records on its device, for eval_groups_device; valid until the next append, rec_tail, rec_sort, rec_clear. */
int  rec_records_device(const rec_store* s, const void** records_device, int64_t* n);
/* Copies the records to the host.  *n always receives the count; DSA_E_CAPACITY if cap is short (nothing is copied). */
int  rec_download(rec_store* s, dsa_record* out, int64_t cap, int64_t* n);
/* The lines of all records in store order (kept == NULL; n_kept is ignored), or of the records kept[0 .. n_kept) in that
 * order: host indices into the store, what eval_groups* returned; an index may repeat.  *bytes always receives the size of
 * the text (64 bits: it can pass 4 GiB); DSA_E_CAPACITY if cap is short, and then out is untouched (and may be NULL).  An
 * index outside the store is DSA_E_ARG, and nothing is written.  No terminating NUL. */
int  rec_text(rec_store* s, const int64_t* kept, int64_t n_kept, char* out, int64_t cap, int64_t* bytes);
int  rec_get_timing(const rec_store* s, rec_timing* out);
const char* rec_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
