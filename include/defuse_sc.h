/*
 * defuse_sc.h — C ABI of the MI355X greedy set cover ("sc") used by the drop-in `setcover` tool.
 *
 * Replaces SetCover(clusters, solution) of the reference (tools/setcover.cpp:30-110): repeatedly
 * take the cluster with the most still-unassigned fragments, assign them to it, and decrement every
 * cluster that contains them.  Among clusters of equal size the one that arrived at that size most
 * recently wins (boost::bimap multiset_of semantics); initial arrival order is
 * ascending cluster index.  The greedy decomposes over the connected components of the
 * cluster/fragment graph, which is what the device exploits: one lane (small components) or one wave
 * (large ones) per component, no global rounds.
 *
 * Plain C types, host pointers.  Returns 0 on success, negative on failure (same codes as defuse_dsa.h).
 */
#ifndef DEFUSE_SC_H_
#define DEFUSE_SC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sc_timing {
    float   build_ms;        /* fragment -> clusters index (radix sort) */
    float   components_ms;   /* connected components (root hooking)    */
    float   greedy_ms;       /* per-component greedy */
    float   total_ms;
    int32_t n_components;
    int32_t n_large;         /* components handled by a whole wave */
    int32_t cc_iterations;
    int32_t pad_;
} sc_timing;

/* clusters are given in CSR form: cluster c owns elements[cluster_off[c] .. cluster_off[c+1]) in file
 * order (duplicates allowed, as in the reference).  owner[e] receives the cluster that fragment e was
 * assigned to, or -1 if e occurs in no cluster; owner must have room for max_element+1 entries. */
int sc_cover(int device, const int64_t* cluster_off, const int32_t* elements, int32_t n_clusters,
             int32_t max_element, int32_t* owner, sc_timing* timing);
const char* sc_last_error(void);
/* Optional: brings the runtime and the device's context up (a few tenths of a second in a fresh process), so that a caller
 * can let that happen on a thread of its own while it parses its input.  Thread-safe; 0, or -2 without a usable device
 * (sc_cover reports that again). */
int sc_prepare(int device);

/* ---- cluster text ------------------------------------------------------------------------------------------------------
 * The text front and back of the set cover ("sct"): the cluster file goes up as text, the filtered cluster file comes down
 * as text, and the caller keeps no parsing rules.  ReadClusters and WriteClusters of the reference (tools/Parsers.cpp:23-170)
 * around SetCover, all on the device; the line tables are built as "defuse_text.h" builds them.  No CPU path: without a
 * device sct_create is DSA_E_DEVICE.  One ctx must not be used from two threads at once.
 *
 * Lines end at '\n'; a '\r' belongs to its field.  Only the first three tab-separated fields of a line matter: clusterID,
 * clusterEnd, fragmentIndex, each by boost::lexical_cast<int> (optional sign, digits only, int range).  Every other byte is
 * copied through or dropped.  A line stops the read pass with the first of these kinds, checked in this order: */
#define SCT_EMPTY_LINE     1          /* length 0                                                                      */
#define SCT_FEW_FIELDS     2          /* fewer than three fields                                                       */
#define SCT_BAD_INTEGER    3          /* one of the three fields is no int                                             */
#define SCT_BAD_CLUSTER_ID 4          /* read pass: clusterEnd == 0 and clusterID < 0; write pass: clusterID < 0       */
/* Outcome of sct_cover (sct_result.status), in the order the reference's two passes impose: */
#define SCT_OK               0
#define SCT_READ_STOP        1        /* the first line in file order with a kind above; it beats everything else      */
#define SCT_NEGATIVE_ELEMENT 2        /* no read stop, but an end-0 line has fragmentIndex < 0                         */
#define SCT_WRITE_STOP       3        /* neither, and a line of any end has clusterID < 0: stop_line is the first such
                                         line, stop_kind is SCT_BAD_CLUSTER_ID, and the out_bytes in front of it are valid */

typedef struct sct_ctx sct_ctx;

typedef struct sct_result {
    int32_t status;          /* SCT_OK ... SCT_WRITE_STOP */
    int32_t stop_kind;       /* SCT_EMPTY_LINE ... of the stopping line, 0 without one */
    int64_t stop_line;       /* 1-based over all pieces, 0 without a stop */
    int64_t stop_offset;     /* the stopping line in the caller's input: the consumed bytes of all pieces back to back */
    int64_t stop_len;        /* its length without the newline */
    int64_t n_lines;         /* lines of all pieces */
    int64_t n_members;       /* end-0 lines */
    int64_t n_clusters;      /* the largest end-0 cluster id + 1 */
    int64_t max_element;     /* the largest end-0 fragment, -1 without one */
    int64_t n_kept_lines;
    int64_t out_bytes;
} sct_result;

typedef struct sct_timing {
    float   upload_ms;       /* the pieces' copies to the device, summed                         */
    float   tables_ms;       /* newline tables of the pieces, summed (with the wait for a count) */
    float   parse_ms;        /* one lane per line: three integers and the stops                  */
    float   layout_ms;       /* end-0 lines -> clusters in CSR form                              */
    float   cover_ms;        /* the set cover                                                    */
    float   select_ms;       /* cluster sizes, keep flags, runs, offsets                         */
    float   gather_ms;       /* the kept lines copied into the output                            */
    float   download_ms;     /* sct_fetch and sct_fetch_owner since the last sct_cover, summed   */
    int64_t text_bytes;      /* consumed bytes of all pieces                                     */
    int64_t gather_bytes;    /* bytes the gather copied (out_bytes less the added newlines)      */
    int64_t n_runs;          /* runs of adjacent kept lines the gather copied                    */
    int32_t n_pieces;
    int32_t n_components;
    int32_t n_large;
    int32_t cc_iterations;
} sct_timing;

int sct_create(int device, sct_ctx** out);
void sct_destroy(sct_ctx* ctx);
/* Empties the ctx: the pieces of the last file and its output go. */
int sct_begin(sct_ctx* ctx);
/* One piece of the cluster file at a host pointer.  final = 0: only whole lines are consumed and *consumed ends behind the
 * last newline (0 without one); the caller gives the rest again in front of its next piece.  final = 1: everything is
 * consumed and a last line without a newline is a line (pieces may follow it: the line ends there, and gains its newline
 * in the output).  Empty text has no line.  len > 2^31 - 1 is DSA_E_LIMIT (found before a device is touched: give the file
 * in pieces), as are more than 2^31 - 1 lines in all pieces.  The consumed bytes stay in device memory until the next
 * sct_begin: the output is gathered from them. */
int sct_add(sct_ctx* ctx, const uint8_t* text, int64_t len, int32_t final, int64_t* consumed);
/* Everything on the pieces given so far: stops, clusters in CSR form, set cover, filter, output bytes.  Returns 0 for every
 * outcome above and says which in r->status.  On SCT_OK and SCT_WRITE_STOP the set cover has run: n_clusters is the largest
 * end-0 cluster id + 1, clusters[id] are the end-0 lines' fragments in file order, and a line of ANY end is kept iff
 * 0 <= clusterID < n_clusters, the cluster owns at least min_cluster_size fragments (a signed 64-bit compare),
 * 0 <= fragmentIndex <= max_element and owner[fragmentIndex] == clusterID.  The output is the kept lines in file order, each
 * followed by '\n' (a kept last line without one gains it).  DSA_E_LIMIT: more than 2^31 - 1 end-0 lines (there cannot be),
 * or a cluster id or fragment of 2^31 - 1 on an end-0 line (the tables would have 2^31 entries). */
int sct_cover(sct_ctx* ctx, int64_t min_cluster_size, sct_result* r);
/* Bytes [offset, offset + len) of the output of the last sct_cover to the host; DSA_E_ARG outside [0, out_bytes]. */
int sct_fetch(sct_ctx* ctx, int64_t offset, uint8_t* buf, int64_t len);
/* owner[0 .. max_element] of the last sct_cover that ran the set cover (none: nothing is written); DSA_E_CAPACITY if cap is
 * smaller than max_element + 1. */
int sct_fetch_owner(sct_ctx* ctx, int32_t* owner, int64_t cap);
int sct_get_timing(const sct_ctx* ctx, sct_timing* out);
const char* sct_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
