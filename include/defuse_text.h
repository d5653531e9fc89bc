/*
 * defuse_text.h — C ABI of the MI355X text front of the split-read chain ("txt"): the improper-mate SAM file and the two
 * FASTQ files go up as text, cand_alignment[] and a read store (bytes + bat_read[]) come out in device memory.
 *
 *     AlignmentStream::GetNextAlignment   tools/AlignmentStream.cpp:39-130   -> txt_parse_sam
 *     FastqReadStream::GetNextRead        tools/ReadStream.cpp:59-103        -> txt_fastq_add
 *     SplitReadRealigner::AddReads        tools/SplitAlignment.cpp:253-264   -> txt_fastq_add + bat_reads_create_device
 *
 * Lines end at '\n'; only '\n' and '\t' are special, a '\r' belongs to the field it is in.  With final = 1 a last line
 * without a newline is a line; with final = 0 it is not consumed.  Empty text has no line.
 *
 * SAM, per line, in this order (the kinds are txt_sam_result.stop_kind):
 *   1. length 0: stop 2.                                 2. first byte '@': the line is skipped.
 *   3. fewer than ten tab-separated fields: stop 3.
 *   4. field 1 (flag) and field 3 (pos) are integers by the rule below, otherwise stop 4.
 *   5. field 2 equal to "*": the line is skipped (after the integer test).
 *   6. strand = (flag & 0x10) ? 1 : 0.
 *   7. a qname with exactly one '/': the part after it must be "1" or "2" (read end 0 / 1), otherwise stop 5; the fragment
 *      is the part before it.  Any other number of slashes: the whole qname is the fragment, the read end is 0 if
 *      flag & 0x40, else 1 if flag & 0x80, else CARRIED from the nearest earlier record of the stream that told it;
 *      carry_in stands for the records of earlier calls, carry_out hands it on.
 *   8. ref = the index of field 2 in the names, or -1.
 *   9. start = pos, end = pos + length(field 9) - 1, formed in 64 bits and truncated to int32.
 *  10. fragment = the fragment text as an integer if it lies in [0, 2^31), otherwise -1.  That is not a stop: see
 *      cand_enumerate_resident.
 * The integer rule (boost::lexical_cast<int>): an optional '+' or '-', then digits only, at least one, value in the int
 * range; leading zeros are fine.
 * A stop ends the stream as the reference's exit(1) does: the records of the lines before stop_line are the result, and
 * `consumed` ends in front of the stopping line.
 *
 * FASTQ: a record is four lines.  With final = 0 only whole groups are consumed; with final = 1 an incomplete last group
 * is dropped silently.  Per record, in this order (txt_fastq_result.stop_kind):
 *   an empty name line or one whose first byte is not '@': stop 1;
 *   the read end is the byte after the first '/': none, or neither '1' nor '2': stop 2;
 *   the fragment is the bytes between '@' and that slash, an integer by the rule above, otherwise stop 3;
 *   a sequence (the second line, whole) of max_read_len (2^24) bases or more: stop 4.
 * A record with a negative fragment is SKIPPED and counted: no candidate can name it and the store's key cannot hold it.
 * A stop ends that file; the records before it stay.  The quality and name bytes are not kept.
 *
 * Plain C types; host pointers unless the name says _device.  Returns 0 on success, negative on failure (codes of
 * defuse_dsa.h).  There is no CPU path: txt_create and txt_names_create fail with DSA_E_DEVICE without a GPU.  Argument
 * errors that can be told from the arguments alone are found before a device is touched.  One object must not be used
 * from two threads at once.  Out of scope: compressed input, more than one GPU per chain.
 */
#ifndef DEFUSE_TEXT_H_
#define DEFUSE_TEXT_H_

#include <stdint.h>

#include "defuse_bat.h"
#include "defuse_cand.h"
#include "defuse_dsa.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TXT_MAX_READ_LEN (1 << 24)     /* the tools' "read longer than 16 M bases"                                      */

#define TXT_SAM_EMPTY_LINE  2          /* stop kinds of a SAM stream: ParseSamLine's return values                      */
#define TXT_SAM_FEW_FIELDS  3
#define TXT_SAM_BAD_INTEGER 4
#define TXT_SAM_BAD_QNAME   5

#define TXT_FASTQ_BAD_NAME     1       /* stop kinds of a FASTQ file                                                    */
#define TXT_FASTQ_BAD_END      2
#define TXT_FASTQ_BAD_FRAGMENT 3
#define TXT_FASTQ_LONG_READ    4

/* What one txt_parse_sam* did. */
typedef struct txt_sam_result {
    int64_t consumed;                  /* bytes up to and including the last consumed line: the next piece starts there */
    int64_t n_lines;                   /* lines consumed, header and skipped ones included, a stopping line not         */
    int64_t n_alignments;              /* records among them                                                            */
    int64_t stop_line;                 /* 1-based within the call (= n_lines + 1), 0 without a stop                     */
    int64_t n_bad_fragment;            /* records whose fragment is -1                                                  */
    int32_t stop_kind;                 /* 0, or TXT_SAM_*                                                               */
    int32_t carry_out;                 /* the carry_in of the next call                                                 */
} txt_sam_result;

/* The alignments of the latest txt_parse_sam* of a ctx on the device.  Valid until the next parse on the ctx or its
 * destruction. */
typedef struct txt_sam_device_view {
    const void* alignments;            /* cand_alignment[n]; a device pointer, never NULL after a successful call       */
    const void* line_of;               /* int32[n]: every record's 1-based line number within the call                  */
    int64_t n;
    int32_t device;
    int32_t pad_;
} txt_sam_device_view;

/* What one txt_fastq_add did. */
typedef struct txt_fastq_result {
    int64_t consumed;                  /* bytes of the whole groups consumed (all of the text with final = 1)           */
    int64_t n_records;                 /* records this call added to the store                                          */
    int64_t n_skipped;                 /* records this call skipped for a negative fragment                             */
    int64_t stop_line;                 /* the stopping name line's number within the FILE (1-based), 0 without a stop   */
    int32_t stop_kind;                 /* 0, or TXT_FASTQ_*                                                             */
    int32_t pad_;
} txt_fastq_result;

/* Everything added since txt_fastq_begin: the sequences back to back in record order and one bat_read per record.  Valid
 * until the next txt_fastq_add or txt_fastq_begin on the ctx or its destruction. */
typedef struct txt_fastq_device_view {
    const void* bytes;                 /* device pointers, never NULL after txt_fastq_begin                             */
    const void* reads;                 /* bat_read[n_reads] {off, len, fragment, read_end, 0}                           */
    int64_t bytes_len;
    int64_t n_reads;
    int32_t device;
    int32_t pad_;
} txt_fastq_device_view;

/* HIP-event times of the most recent txt_parse_sam* or txt_fastq_add of a ctx (the events sit on the ctx's stream and
 * enclose the waits for the two small counts a call brings down), and of the most recent txt_*_fetch after it. */
typedef struct txt_timing {
    float   upload_ms;                 /* the text to the device (a device-to-device copy for txt_parse_sam_device)     */
    float   device_ms;                 /* every kernel and scan of the call                                             */
    float   download_ms;               /* txt_sam_fetch / txt_fastq_fetch                                               */
    float   pad_;
    int64_t text_bytes;                /* bytes the kernels looked at                                                   */
    int64_t n_lines;
    int64_t n_records;
    int64_t gather_bytes;              /* sequence bytes copied (txt_fastq_add)                                         */
} txt_timing;

typedef struct txt_names txt_names;    /* opaque: the reference names of a run on one device, sorted                    */
typedef struct txt_ctx txt_ctx;        /* opaque: one stream and the buffers of one caller, reused call after call      */

/* The caller's dense reference numbering: name k is name_bytes[name_off[k] .. name_off[k + 1]), index = position, the
 * numbering of cand_region.ref.  The names are sorted once; a field is looked up by exact byte comparison.  An empty name
 * is allowed.  DSA_E_ARG for offsets that do not ascend or leave name_bytes (naming the name) and for two equal names
 * (naming both).  n_names > 2^31 - 1 is DSA_E_LIMIT.  Everything is copied. */
int txt_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names,
                     txt_names** out);
void txt_names_destroy(txt_names* names);

int txt_create(int device, txt_ctx** out);
void txt_destroy(txt_ctx* ctx);
/* Lowers (or restores) the sequence length at which a FASTQ file stops with TXT_FASTQ_LONG_READ: 1 .. TXT_MAX_READ_LEN. */
int txt_set_max_read_len(txt_ctx* ctx, int32_t max_read_len);

/* One piece of a SAM stream by the rules at the top.  final and carry_in are 0 / 1.  len > 2^31 - 1 is DSA_E_LIMIT: give
 * the text in pieces.  The alignments stay in the ctx (txt_sam_view); after a failure there are none.
 * txt_parse_sam_device takes the text from device memory of the same GPU; it is copied, so it is free on return. */
int txt_parse_sam(txt_ctx* ctx, const txt_names* names, const uint8_t* text, int64_t len, int32_t final, int32_t carry_in,
                  txt_sam_result* result);
int txt_parse_sam_device(txt_ctx* ctx, const txt_names* names, const void* text_device, int64_t len, int32_t final,
                         int32_t carry_in, txt_sam_result* result);
int txt_sam_view(const txt_ctx* ctx, txt_sam_device_view* out);
/* Downloads the alignments and, if line_cap is not 0, their line numbers (capacities in elements).  DSA_E_CAPACITY if a
 * buffer is short; nothing is written then. */
int txt_sam_fetch(txt_ctx* ctx, cand_alignment* alignments, int64_t cap, int32_t* line_of, int64_t line_cap);

/* txt_fastq_begin empties the store of the ctx.  txt_fastq_add appends the records of one piece of a file; final = 1 ends
 * the file, and the next piece begins the next file (line numbers start at 1 again).  After a stop the further pieces of
 * that file are passed over (consumed = len, the same stop in the result) up to and including the one with final = 1.
 * len > 2^31 - 1 is DSA_E_LIMIT: give the text in pieces. */
int txt_fastq_begin(txt_ctx* ctx);
int txt_fastq_add(txt_ctx* ctx, const uint8_t* text, int64_t len, int32_t final, txt_fastq_result* result);
int txt_fastq_view(const txt_ctx* ctx, txt_fastq_device_view* out);
/* Downloads the bytes and the records.  DSA_E_CAPACITY if a buffer is short; nothing is written then. */
int txt_fastq_fetch(txt_ctx* ctx, uint8_t* bytes, int64_t bytes_cap, bat_read* reads, int64_t reads_cap);

int txt_get_timing(const txt_ctx* ctx, txt_timing* out);
const char* txt_last_error(void);

/* ---- the consumers' device-pointer twins (implemented next to their host forms) ------------------------------------- */

/* cand_enumerate_device (defuse_bat.h) for alignments in device memory of the session's GPU (txt_sam_view).  What the host
 * form checks on the host a kernel checks here: a strand or read_end outside 0 / 1 is DSA_E_ARG, naming the lowest index.
 * An alignment with fragment < 0 that overlaps nothing is passed over, as the reference casts the fragment only inside the
 * loop over the overlapping ids (tools/SplitAlignment.cpp:281).  The lowest alignment with fragment < 0 that does overlap
 * something fails the call with DSA_E_ARG: *first_bad is its index (-1 otherwise) and the session stays as it was, so the
 * caller enumerates the alignments before it and ends with the reference's message.  Messages: cand_last_error.  The
 * records stay resident for cand_records_device. */
int cand_enumerate_resident(cand_session* session, const void* alignments_device, int64_t n, int32_t order, int64_t* n_out,
                            int64_t* first_bad, cand_timing* timing);

/* bat_reads_create (defuse_bat.h) from device memory of `device` (txt_fastq_view): the per-record checks run in a kernel
 * that reports the lowest bad record (DSA_E_ARG, the message of bat_last_error names it).  The store copies the bytes. */
int bat_reads_create_device(int device, const void* bytes_device, int64_t bytes_len, const void* reads_device, int64_t n,
                            bat_reads** out);

#ifdef __cplusplus
}
#endif
#endif
