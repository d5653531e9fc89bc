/*
 * defuse_cmp.h — C ABI of the MI355X bin-pair builder ("cmp" = clustermatepairs) of the drop-in `clustermatepairs` tool.
 *
 * Replaces the front half of the reference tool's main loop for all fragments of the input at once
 * (tools/clustermatepairs.cpp:453-476): per fragment
 *
 *     CheckConcordant(alignments, minFusionRange)            tools/clustermatepairs.cpp:211-244
 *       -> Binning::GetBins with length = extend = minFusionRange   :146-176   (C++ int division)
 *     AddBinPairs(alignments, Binning(1 << 15, minFusionRange), binPairs)      :246-290
 *       -> PackAlignment (relative positions in 16 bits, DebugChecks)          :178-192
 *       -> RefBinPacked (18 bits reference, 1 bit strand, 13 bits bin)         :28-65
 *
 * and the unordered_map of bin pairs those calls fill.  On the device: one thread per fragment decides concordance and
 * counts, a scan gives every fragment its place, a second pass writes (bin-pair key, packed alignment) entries for the
 * `first` and the `second` list of every bin pair, and a stable radix sort by key — entries arrive in file order, so a
 * stable sort leaves every list in the order a serial reader would have appended it — turns them into the bin pairs in
 * ascending key order, the canonical visiting order of SURVEY.md 8(c).
 *
 * Plain C types, host pointers, caller-owned buffers.  Returns 0 on success, negative on failure (codes of defuse_dsa.h).
 */
#ifndef DEFUSE_CMP_H_
#define DEFUSE_CMP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One line of the compact alignment input (tools/AlignmentStream.cpp:156-199), reference names replaced by their index in
 * order of first appearance.  Records of one fragment are consecutive (FragmentAlignmentStream, :201-221). */
typedef struct cmp_record {
    int32_t  fragment;          /* readID.fragmentIndex */
    int32_t  start, end;        /* region */
    uint32_t meta;              /* reference index (bits 0-27) | strand << 28 | read end << 29 */
} cmp_record;
#define CMP_META(ref, strand, read_end) ((uint32_t)(ref) | ((uint32_t)(strand) << 28) | ((uint32_t)(read_end) << 29))

/* AlignmentPacked (tools/clustermatepairs.cpp:67-78): what a bin pair's lists hold */
typedef struct cmp_packed {
    int32_t  fragment, read_end;
    uint16_t rel_start, rel_end;
} cmp_packed;

typedef struct cmp_stats {
    int64_t n_fragments, n_concordant;
    int64_t n_keys;             /* bin pairs */
    int64_t n_first, n_second;  /* entries of all `first` / all `second` lists */
    /* the first alignment (in file order) on which the reference would have stopped, -1 if none:
     * kind 1 = DebugCheck of PackAlignment (relative position outside 16 bits), 2 = "Packing failed, too many reference
     * sequences" (value = the reference index), 3 = "Packing failed, chromosome too large" (value = the bin) */
    int64_t err_record;
    int32_t err_kind, err_value;
    float   device_ms;          /* kernels and sorts, HIP events */
    float   pad_;
} cmp_stats;

typedef struct cmp_binner cmp_binner;
int  cmp_bin_create(cmp_binner** out, int device);          /* fails without a GPU: there is no CPU path */
void cmp_bin_destroy(cmp_binner* b);
/* room for the whole input on the device; then the records and the fragment starts may be uploaded in pieces (from several
 * host threads if the caller parsed in pieces): records [at, at + n), and frag_start values — the index of every fragment's
 * first record, the caller adds one more entry = n_records at the end */
int  cmp_bin_reserve(cmp_binner* b, int64_t n_records, int64_t n_fragments);
int  cmp_bin_upload_records(cmp_binner* b, const cmp_record* recs, int64_t n, int64_t at);
int  cmp_bin_upload_fragments(cmp_binner* b, const uint32_t* frag_start, int64_t n, int64_t at);
/* everything on the device; the counts tell the caller how much room cmp_bin_fetch needs */
int  cmp_bin_run(cmp_binner* b, int32_t min_fusion_range, cmp_stats* stats);
/* bin pair k: key = (first.id << 32) | second.id (RefBinPacked ids), ascending; its lists are
 * first[off_first[k] .. off_first[k+1]) and second[off_second[k] .. off_second[k+1]) (n_keys + 1 offsets each) */
int  cmp_bin_fetch(cmp_binner* b, uint64_t* keys, int64_t* off_first, int64_t* off_second, cmp_packed* first, cmp_packed* second);
/* entries [from, from + n) of all `first` (which = 0) or all `second` (1) lists: a caller with several host threads passes
 * NULL for the lists above and lets every thread copy its own share into memory it touches for the first time itself */
int  cmp_bin_fetch_part(cmp_binner* b, int which, int64_t from, int64_t n, cmp_packed* out);
const char* cmp_last_error(void);

/* ---- The EM problems of the bin pairs, built on the device ---------------------------------------------------------
 *
 * What the tool's host stages do between the bin pairs and MatePairEM (tools/clustermatepairs.cpp:478-545 with :292-375),
 * for all bin pairs at once and with the same result bit for bit: bin pairs whose two lists both hold at least
 * min_cluster_size entries are candidates; per side the entries of a candidate are grouped by fragment (fragments
 * ascending as signed int, list order inside a fragment, wherever in the list its entries lie); fragments absent from the
 * other side go (FilterUnmatched); per fragment an alignment is kept only if no alignment kept before it, of the same read
 * end, reaches one of its minFusionRange bins (FilterOverlapping; bins by C++ truncating division); a bin pair with at
 * least min_cluster_size matched fragments is a problem.  Its mate pairs are, fragment by fragment, the kept alignments of
 * `first` in list order times those of `second` in list order (GetAlignPairs); per mate pair x = r1.end, y = r2.end,
 * u = (fragment_mean - len1) - len2 on the strand-remapped regions, and to_xo / to_yo the rank inside the problem by x
 * (y) descending, ties by index ascending — the arrays mpe_cluster_batch takes.  Problems come in ascending key order.
 *
 * Limits (DSA_E_LIMIT): a problem of more than INT32_MAX mate pairs, or more than INT32_MAX mate pairs in one build. */
typedef struct cmp_problem_counts {
    int64_t n_candidates;       /* bin pairs with both lists >= min_cluster_size */
    int64_t n_problems, n_mate_pairs;
    float   device_ms;          /* kernels, sorts and scans, HIP events */
    float   pad_;
} cmp_problem_counts;

/* alignPairs: indices into the `first` and the `second` list of the problem's bin pair */
typedef struct cmp_pair { int32_t first, second; } cmp_pair;

/* One printed cluster member (OutputClusterMember, tools/clustermatepairs.cpp:549-583): index 0 = the alignment of
 * `first` (cluster end 0), 1 = that of `second`.  ref is the reference index of the records, strand 0 plus / 1 minus. */
typedef struct cmp_row {
    int32_t cluster_id;
    int32_t fragment[2], read_end[2], ref[2], strand[2], start[2], end[2];
} cmp_row;

/* the arrays on the device (device pointers; valid until the next build on the object or its destruction) */
typedef struct cmp_problems_device {
    const int64_t*  prob_off;   /* n_problems + 1 */
    const double    *x, *y, *u; /* n_mate_pairs each */
    const int32_t   *to_xo, *to_yo;
    const cmp_pair* pairs;
    const int32_t*  bin_pair;   /* n_problems: the index of the problem's bin pair among the keys */
    uint16_t*       member;     /* room for n_mate_pairs masks: where mpe_cluster_batch_device may write, for cmp_problems_select */
    int64_t n_problems, n_mate_pairs;
    int32_t device, pad_;
} cmp_problems_device;

typedef struct cmp_problems cmp_problems;
int  cmp_problems_create(cmp_problems** out, int device);
void cmp_problems_destroy(cmp_problems* p);
/* From what cmp_bin_run left on the binner's device (no cmp_bin_fetch needed).  The lists are read in place, also by
 * cmp_problems_select afterwards: the binner has to stay alive, and unchanged, as long as this object is used.  The
 * binner and the object must be on the same device. */
int  cmp_problems_build(cmp_problems* p, cmp_binner* b, int32_t min_fusion_range, int32_t min_cluster_size, double fragment_mean,
                        cmp_problem_counts* counts);
/* The same from lists in host memory, in the layout cmp_bin_fetch hands out (keys ascending and distinct, n_keys + 1
 * offsets per side): they are uploaded and go through the same kernels. */
int  cmp_problems_build_lists(cmp_problems* p, const uint64_t* keys, const int64_t* off_first, const int64_t* off_second,
                              const cmp_packed* first, const cmp_packed* second, int64_t n_keys, int32_t min_fusion_range,
                              int32_t min_cluster_size, double fragment_mean, cmp_problem_counts* counts);
/* Any subset of the arrays to the host (NULL = not wanted); sizes as in cmp_problems_device. */
int  cmp_problems_fetch(cmp_problems* p, int64_t* prob_off, double* x, double* y, double* u, int32_t* to_xo, int32_t* to_yo,
                        cmp_pair* pairs, int32_t* bin_pair);
/* The build has completed on the device when cmp_problems_build* returns: the pointers can be used from any stream. */
int  cmp_problems_view(const cmp_problems* p, cmp_problems_device* out);
/* The lines to print of problems [p0, p1), chosen on the device.  n_clusters (host) holds p1 - p0 counts, n_clusters[0]
 * that of problem p0; member (DEVICE pointer) holds the masks of their mate pairs, member[0] that of mate pair
 * prob_off[p0] — what mpe_cluster_batch_device wrote.  For cluster j < n_clusters[p] a mate pair is selected when its bit
 * j is set and no earlier mate pair of the same fragment in that problem has bit j set; bits from n_clusters[p] up are
 * ignored.  Rows come by problem, then cluster, then mate pair; cluster_id = cluster_base + (sum of n_clusters of the
 * problems of the range before p) + j.  The rows stay on the device until the next select; *n_rows receives their number. */
int  cmp_problems_select(cmp_problems* p, int64_t p0, int64_t p1, const int32_t* n_clusters, const uint16_t* member,
                         int32_t cluster_base, int64_t* n_rows);
/* The rows of the last select.  *n_rows always receives their number; DSA_E_CAPACITY if cap is short (nothing is copied,
 * rows may then be NULL). */
int  cmp_problems_rows(cmp_problems* p, cmp_row* rows, int64_t cap, int64_t* n_rows);

/* ---- Alignment and cluster text ("cmpt") ------------------------------------------------------------------------------
 *
 * The text on both sides of the objects above, on the device: the compact alignment file goes up as text and becomes the
 * records, fragment starts and reference names the binner takes (CompactAlignmentStream and FragmentAlignmentStream,
 * tools/AlignmentStream.cpp:156-221, with the name numbering of tools/clustermatepairs.cpp:430-446), and the rows of
 * cmp_problems_select become the lines of the cluster file (OutputClusterMember, tools/clustermatepairs.cpp:376-387).
 *
 * Parse.  The text comes in pieces of at most 2^31 - 1 bytes.  Lines end at '\n' ('\r' belongs to its field).  With
 * final = 0 an open last line is not consumed and `consumed` says where the next piece starts; with final = 1 it is a
 * line.  Per line, in this order: length 0 stops with CMPT_EMPTY_LINE; fewer than six tab-separated fields with
 * CMPT_FORMAT; a field 0 that is no integer (optional sign, digits only, int range) with CMPT_BAD_FRAGMENT; such a field
 * 4 or 5 with CMPT_BAD_POSITION.  Fields behind the sixth are ignored.  The record is {fragment, start, end,
 * CMP_META(ref, strand, read_end)} with read_end = (field 1 is "1") ? 0 : 1, strand = (field 3 is "-") ? 1 : 0 and ref the
 * index of field 2 among the distinct names of the stream in order of first appearance, compared as exact bytes (an empty
 * name is a name).  A line starts a fragment when the BYTES of its field 0 differ from those of the line before it ("7",
 * "07" and "+7" are three fragments); the last line's field 0 is carried from piece to piece.  A stop ends the stream:
 * records, fragments and names are those of the lines before it, and later pieces are passed over (consumed whole).
 *
 * Limits (DSA_E_LIMIT): a piece of more than 2^31 - 1 bytes, more than 2^32 - 1 records, more than max_names distinct
 * names.  After a failed cmpt_add the stream is over: cmpt_begin starts the next one on the same context.
 *
 * Print.  Two lines per cmp_row, end 0 and then end 1:
 *     cluster_id \t end \t fragment \t read_end \t name \t +|- \t start \t end \n
 * integers as operator<<(int) prints them, names from the context's dictionary, strand 0 as '+' and any other as '-'.
 * A ref outside the dictionary is DSA_E_ARG, and bad_row names the lowest such row.
 *
 * cmpt_last_error() has the text of a failed cmpt_ call on a context; the three entries that take a cmp_binner or a
 * cmp_problems report through cmp_last_error(). */
#define CMPT_EMPTY_LINE   1
#define CMPT_FORMAT       2
#define CMPT_BAD_FRAGMENT 3
#define CMPT_BAD_POSITION 4

typedef struct cmpt_result {
    int64_t consumed;                           /* bytes of this piece that were taken */
    int64_t n_lines;                            /* of the whole stream so far: lines read (a stopping line included), */
    int64_t n_records, n_fragments, n_names;    /*   records, fragments and names */
    int64_t stop_line;                          /* 1-based in the whole stream; 0 = no stop */
    int64_t stop_offset, stop_len;              /* where the stopping line lies in the stream's bytes, without its newline */
    int32_t stop_kind, pad_;                    /* CMPT_* */
} cmpt_result;

/* what the parse left on the device (device pointers; valid until the next cmpt_add or cmpt_begin on the context) */
typedef struct cmpt_device {
    const cmp_record* records;                  /* n_records */
    const uint32_t*   frag_start;               /* n_fragments + 1, closed by n_records */
    const uint8_t*    name_bytes;               /* the names one behind the other */
    const int64_t*    name_off;                 /* n_names + 1 */
    int64_t n_records, n_fragments, n_names, n_name_bytes;
    int32_t device, pad_;
} cmpt_device;

typedef struct cmpt_print_result {
    int64_t n_rows, text_bytes;
    int64_t bad_row;                            /* the lowest row with a ref outside the dictionary, -1 if none */
} cmpt_print_result;

/* HIP-event times, summed over the pieces of a stream (parse) and of the latest print */
typedef struct cmpt_timing {
    float   upload_ms, tables_ms, lines_ms, names_ms, layout_ms;      /* parse */
    float   lengths_ms, write_ms, download_ms;                         /* print: lengths + scan, write, cmpt_text_fetch */
    int64_t text_bytes, out_bytes;
    int32_t n_pieces, pad_;
} cmpt_timing;

typedef struct cmpt_ctx cmpt_ctx;
/* max_names in [1, 2^28]: the name table is a power of two of at least twice it.  Fails without a GPU. */
int  cmpt_create(int device, int64_t max_names, cmpt_ctx** out);
void cmpt_destroy(cmpt_ctx* c);
int  cmpt_begin(cmpt_ctx* c);
int  cmpt_add(cmpt_ctx* c, const uint8_t* text, int64_t len, int32_t final, cmpt_result* result);
/* the same for text in device memory (on the context's device; it is copied, and needs no padding) */
int  cmpt_add_device(cmpt_ctx* c, const uint8_t* text_device, int64_t len, int32_t final, cmpt_result* result);
int  cmpt_view(const cmpt_ctx* c, cmpt_device* out);
/* records (room for n_records) and fragment starts (room for n_fragments + 1) to the host; NULL = not wanted;
 * DSA_E_CAPACITY if a wanted buffer is short */
int  cmpt_fetch(cmpt_ctx* c, cmp_record* records, int64_t record_cap, uint32_t* frag_start, int64_t frag_cap);
/* the names' bytes and n_names + 1 offsets; NULL = not wanted; DSA_E_CAPACITY as above */
int  cmpt_names_fetch(cmpt_ctx* c, uint8_t* bytes, int64_t byte_cap, int64_t* off, int64_t off_cap);
/* The device-pointer twins of cmp_bin_upload_records and cmp_bin_upload_fragments: device-to-device copies into what
 * cmp_bin_reserve reserved, from memory on the binner's device (a cmpt_view, for one).  Complete on return. */
int  cmpt_bin_upload_records_device(cmp_binner* b, const cmp_record* records_device, int64_t n, int64_t at);
int  cmpt_bin_upload_fragments_device(cmp_binner* b, const uint32_t* frag_start_device, int64_t n, int64_t at);
/* The rows of the last cmp_problems_select where they are (valid until the next select on the object). */
int  cmpt_problems_rows_view(cmp_problems* p, const cmp_row** rows_device, int64_t* n_rows);
/* The lines of n_rows rows (host memory / memory of the context's device) into the context; n_rows = 0 is empty text. */
int  cmpt_print_rows(cmpt_ctx* c, const cmp_row* rows, int64_t n_rows, cmpt_print_result* result);
int  cmpt_print_rows_device(cmpt_ctx* c, const cmp_row* rows_device, int64_t n_rows, cmpt_print_result* result);
/* The text of the last print.  *n_bytes always receives its size; DSA_E_CAPACITY if cap is short (nothing is copied). */
int  cmpt_text_fetch(cmpt_ctx* c, uint8_t* buf, int64_t cap, int64_t* n_bytes);
int  cmpt_get_timing(const cmpt_ctx* c, cmpt_timing* out);
const char* cmpt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
