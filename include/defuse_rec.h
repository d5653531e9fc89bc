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

/* ---- alignment text ---------------------------------------------------------------------------------------------------
 * The way into a store for an alignment FILE (splitreads.alignments, what SplitAlignment::ReadSortedAlignments reads,
 * tools/SplitAlignment.cpp:319-369): rect_add parses one piece of the text on the device and appends the records of its lines
 * behind the store's last record.  Text up, rec_sort, rec_text down is `LC_ALL=C sort -n -k 1 FILE...` for files of plain
 * lines (below), and for sorted inputs also `sort -m -n -k 1`: GNU sort's last-resort comparison makes its order total up to
 * identical lines.
 *
 * Lines.  Only '\n' and '\t' are special; a '\r' belongs to the field it is in.  With final = 1 a last line without a newline
 * is a line; with final = 0 it is not consumed (the caller gives it again in front of the next piece).  Empty text has no line.
 *
 * Per line, in this order:
 *   1. Fewer than nine tab-separated fields: stop RECT_FEW_FIELDS, stop_field = -1.  An empty line has one field and stops
 *      here.  (The reference tests "< 7" and then indexes [8]; the host parser of tools_src/evaluate.hpp stops below nine.)
 *   2. Fields 0 to 8 are checked in order; the first failing field decides the stop kind, and stop_field is its index.
 *      Field 3 must be exactly "0" or "1" (lexical_cast<bool>), else RECT_BAD_BOOL.  Every other field must be an integer,
 *      else RECT_BAD_INTEGER: an optional '+' or '-', then digits only, at least one, and a value in the int range; leading
 *      zeros are fine (field_int of tools_src/defuse_host.hpp).
 *   3. Fields beyond the ninth are ignored.
 *   4. The record is dsa_record{fusion_id, frag, read_end, revcomp, ref_first, ref_second, read_first, read_second, score,
 *      pair_idx = 0} from fields 0 to 8.
 *   5. A line is PLAIN if its bytes, without the newline, are exactly what rec_text prints for its record: nine "%d\t".
 *      "+7", "007", "-0", a missing last tab, an extra field and a trailing '\r' all make a line parse but not be plain.
 *      Lines that are not plain still give records; they are counted, because printing their records would not give their
 *      bytes back and GNU sort's numeric key reads them differently.
 *
 * Stop.  A stop ends the stream, as the reference's exit(1) does: the lowest stopping line wins, the records of the lines
 * before it are appended, and `consumed` ends in front of it.
 *
 * The conventions of this header hold.  Argument errors that can be told from the arguments alone are found before a device
 * is touched.  len > 2^31 - 1 is DSA_E_LIMIT: the caller gives the text in pieces.  A store that would pass its record bound
 * is DSA_E_LIMIT, and nothing is appended.  The ctx and the store must be on one device, else DSA_E_ARG.
 */
#define RECT_FEW_FIELDS  1            /* fewer than nine fields                                                          */
#define RECT_BAD_INTEGER 2            /* a field other than the fourth is no int                                         */
#define RECT_BAD_BOOL    3            /* the fourth field is not "0" or "1"                                              */

typedef struct rect_result {
    int64_t consumed;        /* bytes of the piece that are dealt with: up to the stopping line, else all whole lines     */
    int64_t n_lines;         /* lines consumed (those in front of a stop)                                                 */
    int64_t n_records;       /* records appended: one per consumed line                                                   */
    int64_t stop_line;       /* 1-based within the call; 0 without a stop                                                 */
    int64_t n_other;         /* lines among the consumed ones that are not plain                                          */
    int64_t first_other;     /* 1-based line of the first of them; 0 if there is none                                     */
    int32_t stop_kind;       /* RECT_FEW_FIELDS ... of the stopping line; 0 without a stop                                */
    int32_t stop_field;      /* index of the field that stopped; -1 for RECT_FEW_FIELDS and without a stop                */
    int32_t stop_id_read;    /* 1 if the stopping line has at least seven fields and field 0 is an integer: what
                                ReadSortedAlignments' look-ahead has checked before it decides that a line opens the next
                                group, so an evalsplitalign caller knows whether the running group is still evaluated     */
    int32_t stop_id;         /* that integer; 0 without it                                                                */
} rect_result;

typedef struct rect_timing { /* HIP events, of the most recent rect_add                                                   */
    float   upload_ms;       /* the text to the device                                                                    */
    float   device_ms;       /* tables, the per-line kernel and the result                                                */
    int64_t text_bytes;      /* bytes sent up (with final = 0: up to the last newline)                                    */
    int64_t n_lines;
    int64_t n_records;
} rect_timing;

typedef struct rect_ctx rect_ctx;     /* opaque: the text buffers and tables of one device; not for two threads at once */

int  rect_create(int device, rect_ctx** out);
void rect_destroy(rect_ctx* ctx);
/* Parses text[0 .. len) and appends to `store` (whatever it holds stays, and keeps its place).  *result is always written. */
int  rect_add(rect_ctx* ctx, rec_store* store, const uint8_t* text, int64_t len, int32_t final, rect_result* result);
int  rect_get_timing(const rect_ctx* ctx, rect_timing* out);
const char* rect_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
