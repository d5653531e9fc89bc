/*
 * defuse_est.h — C ABI of the MI355X EST island catalogue behind the drop-in `estislands` tool.
 *
 * Replaces EstCatalog (tools/EstCatalog.cpp): the EST alignments of every chromosome sorted by start and merged into
 * islands (SortAndMergeSegments, :72-101), and the test whether a breakpoint alignment lies inside an island padded by
 * EST_ISLAND_PAD bases on either side (FilterContainedInEstIslands, :103-173).
 *
 * Segments are sorted by (chromosome, start, position in the input): a stable sort.  When every segment has end >= start
 * the islands do not depend on how equal starts are ordered (proof in est_api.hip), so they equal the reference's for
 * any std::sort.  A segment with end < start makes the sequential merge order-dependent; for it this order is the
 * canonical one, and the islands are exactly what the reference's loop computes on the segments in this order —
 * including a degenerate first segment of a chromosome, which that loop emits twice.
 *
 * Lookup: lower_bound by start among the chromosome's islands, one step back unless at the first, then a forward walk
 * while island.start <= q.end; q is contained if some visited island has start - PAD <= q.start and end + PAD >= q.end.
 * Islands that start after q.end are never visited, whatever their padding.  The padded bounds are computed in 64 bits;
 * the reference computes them in int, so they differ only for island coordinates within PAD of INT_MIN or INT_MAX, where
 * the reference's arithmetic overflows.
 *
 * Plain C types, host pointers.  Returns 0 on success, negative on failure (codes of defuse_dsa.h).
 */
#ifndef DEFUSE_EST_H_
#define DEFUSE_EST_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EST_ISLAND_PAD 300     /* tools/EstCatalog.cpp:157-158 */

typedef struct est_timing {
    float   build_ms;          /* est_catalog_create: upload, sort, islands (HIP events)  */
    float   lookup_ms;         /* est_catalog_contained: upload, search, download         */
    int64_t n_segments;        /* EST alignments in the catalogue                         */
    int64_t n_degenerate;      /* of them with end < start                                */
    int64_t n_islands;
    int64_t n_queries;         /* of the last est_catalog_contained                       */
    int64_t n_contained;
} est_timing;

typedef struct est_catalog est_catalog;   /* opaque: the islands of one catalogue on one device */

/* Segments as columns: chrom[k] in [0, n_chrom) is a dense chromosome id, start/end as the reference computes them
 * (int(tStart) + 1, int(tEnd)).  n may be 0; chromosomes without segments have no islands.  *out is freed by
 * est_catalog_destroy.  Fails (DSA_E_DEVICE) without a GPU: there is no CPU path. */
int est_catalog_create(int device, const int32_t* chrom, const int32_t* start, const int32_t* end, int64_t n, int32_t n_chrom,
                       est_catalog** out);
/* The islands in order, chromosome by chromosome: chromosome c owns [chrom_off[c], chrom_off[c+1]) (n_chrom + 1 entries).
 * *n_islands receives the count; if it exceeds cap the call returns DSA_E_CAPACITY and writes nothing else. */
int est_catalog_islands(est_catalog* cat, int32_t* start, int32_t* end, int64_t cap, int64_t* n_islands, int64_t* chrom_off);
/* contained[k] = 1 if query k lies in a padded island of chromosome chrom[k], else 0.  A chrom outside [0, n_chrom) has
 * no islands.  timing may be NULL. */
int est_catalog_contained(est_catalog* cat, const int32_t* chrom, const int32_t* start, const int32_t* end, int64_t n,
                          uint8_t* contained, est_timing* timing);
void est_catalog_destroy(est_catalog* cat);
const char* est_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
