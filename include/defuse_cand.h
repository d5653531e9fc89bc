/*
 * defuse_cand.h — C ABI of the MI355X candidate enumeration in front of the split-read DP ("cand").
 *
 * Replaces the candidate loop of SplitReadRealigner::DoAlignment (tools/SplitAlignment.cpp:266-303) for a whole batch
 * of improper mate alignments at once:
 *
 *     BinnedLocations::Add          tools/SplitAlignment.cpp:177-195    -> cand_table_create
 *     BinnedLocations::Overlapping  tools/SplitAlignment.cpp:197-229    -> cand_enumerate, per alignment
 *     the candidate of a hit        tools/SplitAlignment.cpp:281-284    -> cand_record
 *     candidateUnique               tools/SplitAlignment.cpp:268, :292  -> the session's seen keys
 *
 * Reference names are dense int32 indices the caller hands out; one numbering covers the regions and the alignments,
 * and an alignment with ref < 0 ("a name the table does not have") overlaps nothing.  Strand is 0 (+) / 1 (-).
 *
 * Bins: a region is entered into bins start / spacing ... end / spacing with C++ int division (truncation toward
 * zero), as BinnedLocations::Add does; a region whose first bin is above its last is in no bin and is never found,
 * whatever its coordinates.  An alignment looks into bins start / spacing ... end / spacing (none if the first is above
 * the last), tests every entry with region.start <= a.end && region.end >= a.start, and yields each id once.
 *
 * Order: the reference iterates an unordered_set of ids; here the ids of an alignment are visited ascending as signed
 * int (the canonical order of SURVEY 8(c)): ids of cluster end 1 are negative and come first.  Candidates are visited
 * in ascending (alignment index, id) and kept first come, first kept.
 *
 * Plain C types, host pointers.  Returns 0 on success, negative on failure (codes of defuse_dsa.h).  There is no CPU
 * path: creating a table fails with DSA_E_DEVICE without a GPU.  Argument errors are found before a device is touched.
 */
#ifndef DEFUSE_CAND_H_
#define DEFUSE_CAND_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAND_BIN_SPACING 2000          /* tools/SplitAlignment.cpp:232 */

#define CAND_ORDER_VISIT   0           /* ascending (alignment, id): the order DoAlignment meets them            */
#define CAND_ORDER_FUSION  1           /* stable by fusion_id, visiting order inside a fusion: what dsa_* wants   */

/* One mate region of a fusion's cluster end (SplitAlignmentTask::mMateRegions[end][k]). */
typedef struct cand_region {
    int32_t ref;                       /* dense reference index, >= 0                                           */
    int32_t strand;                    /* 0 / 1                                                                 */
    int32_t start, end;                /* as the reference stores them; end < start is allowed                  */
    int32_t id;                        /* ClusterID.id: fusion id in bits 0-30, cluster end in bit 31, signed   */
} cand_region;

/* One improper mate alignment (a record of the SAM stream, tools/AlignmentStream.cpp:39-130). */
typedef struct cand_alignment {
    int32_t ref;                       /* dense reference index, < 0: not in the table                          */
    int32_t strand;                    /* 0 / 1                                                                 */
    int32_t start, end;
    int32_t fragment;                  /* ReadID.fragmentIndex, in [0, 2^31)                                    */
    int32_t read_end;                  /* the mate's own read end, 0 / 1                                        */
} cand_alignment;

/* One kept candidate (fusion, read, revComp): what DoAlignment hands to SplitAlignmentTask::Align. */
typedef struct cand_record {
    int64_t alignment;                 /* index of its alignment in the session: alignments of earlier calls + k */
    int32_t fusion_id;                 /* id & 0x7FFFFFFF                                                       */
    int32_t fragment;
    uint8_t cluster_end;               /* id < 0                                                                */
    uint8_t read_end;                  /* of the read to align: the other end than the mate's                   */
    uint8_t revcomp;                   /* cluster_end == 0                                                      */
    uint8_t first;                     /* 1 on the first kept candidate of its alignment (in visiting order)    */
    uint8_t pad_[4];
} cand_record;

typedef struct cand_timing {
    float   upload_ms;                 /* alignments to the device (HIP events on the session's stream)         */
    float   device_ms;                 /* every kernel, sort and scan of the call                               */
    float   download_ms;               /* records to the host                                                   */
    float   pad_;
    int64_t n_alignments;              /* of this call                                                          */
    int64_t n_hits;                    /* (alignment, table entry) overlaps, before the per-alignment uniquing  */
    int64_t n_visited;                 /* distinct (alignment, id)                                              */
    int64_t n_kept;                    /* candidates that were not kept before in this session                  */
} cand_timing;

typedef struct cand_table cand_table;       /* opaque: the binned mate regions on one device              */
typedef struct cand_session cand_session;   /* opaque: the keys kept so far in one DoAlignment run        */

/* id = fusion_id + (cluster_end << 31) as a signed int (ClusterID, tools/Common.h:206-218).  DSA_E_ARG if fusion_id
 * is outside [0, 2^31) or cluster_end is not 0 / 1: such an id would be taken for another fusion's. */
int cand_cluster_id(int64_t fusion_id, int32_t cluster_end, int32_t* id);

/* BinnedLocations::Add for all regions.  bin_spacing > 0 (CAND_BIN_SPACING for the reference); n may be 0.  The number
 * of (region, bin) entries is the sum over the regions of last bin - first bin + 1; above 2^31 - 1 the call fails with
 * DSA_E_LIMIT before anything is allocated.  *out is freed by cand_table_destroy, after the sessions on it. */
int cand_table_create(int device, const cand_region* regions, int64_t n, int32_t bin_spacing, cand_table** out);
void cand_table_destroy(cand_table* table);

/* A session holds what one run of DoAlignment has kept so far and counts the alignments it was given.  Several
 * sessions may share a table; they do not see each other.  One session must not be used from two threads at once. */
int cand_session_create(cand_table* table, cand_session** out);
int cand_session_reset(cand_session* session);       /* forgets every key, the count starts at 0 again */
void cand_session_destroy(cand_session* session);

/* The candidates of alignments[0..n) in `order`.  *n_out always receives their number; if it exceeds cap the call
 * returns DSA_E_CAPACITY, writes nothing else and leaves the session as it was (seen keys and count), so that the same
 * call with room succeeds.  n >= 2^31, or more than 2^31 - 1 hits in one call, is DSA_E_LIMIT: give fewer alignments
 * per call.  The alignments are checked (strand, read_end, fragment) before the session is looked at.  timing may be
 * NULL. */
int cand_enumerate(cand_session* session, const cand_alignment* alignments, int64_t n, int32_t order,
                   cand_record* out, int64_t cap, int64_t* n_out, cand_timing* timing);

/* The device-pointer twins of cand_enumerate, which leave the records in the session's device buffer for the batch
 * assembly, are declared next to their consumer in defuse_bat.h. */
const char* cand_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
