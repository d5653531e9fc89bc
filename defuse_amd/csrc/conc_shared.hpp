// conc_shared.hpp — the rules of prep_local_alignment_seqs.pl over flattened gene models (include/defuse_task.h, section "concordant clusters"), as
// __host__ __device__ code: the kernels of conc_api.hip and a host program (tests/test_conc_filter.py) compile the same functions.
//
// Positions are doubled ("half-units", names ending in 2): the midpoint (start + end) / 2 is start + end.  With coordinates within
// +-TASK_MAX_COORD and a range within TASK_MAX_PARAM every value stays far inside an int64.
#pragma once
#include <stdint.h>

#include "../../include/defuse_task.h"

#if defined(__HIPCC__)
#define CONC_HD __host__ __device__ inline
#else
#define CONC_HD inline
#endif

// the models and the reference's tables where the caller has them (device or host pointers)
struct conc_view {
    const conc_gene* genes;
    const int32_t* gene_tx;
    const conc_transcript* tx;
    const conc_interval* exons;
    const conc_interval* expr;
    const int32_t* chrom_gene_first;
    const int32_t* chrom_genes;
    const int32_t* chrom_premax;        // beside chrom_genes: the greatest region end up to and including that gene
    const uint8_t* names;
    const conc_name* chrom_names;
    const conc_name* tx_names;
    const conc_name* seq_names;
    const int32_t* seq_sorted;          // the sequences ascending by name bytes
    const int32_t* chrom_seq;           // the sequence a chromosome / a transcript is, -1 where the FASTA lacks it
    const int32_t* tx_seq;
    const task_seq* seqs;
    int32_t n_chroms, n_tx, n_seqs, pad_;
};

CONC_HD int conc_name_cmp(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb)
{
    const int64_t n = la < lb ? la : lb;
    for (int64_t k = 0; k < n; ++k)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// the entry of an ascending table (through `perm` where it is given) that equals q, else -1
CONC_HD int32_t conc_find_name(const uint8_t* names, const conc_name* table, const int32_t* perm, int32_t n, const uint8_t* q, int64_t lq)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const int32_t k = perm ? perm[mid] : mid;
        const int c = conc_name_cmp(names + table[k].off, table[k].len, q, lq);
        if (c == 0) return k;
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// Fasta.pm:905: /^(.+):([\d_]+)(?:,|-|\.\.)([\d_]+)$/ (the classes exclude the separators, so either run is the longest one)
CONC_HD bool conc_name_is_range(const uint8_t* s, int64_t n)
{
    auto digit = [](uint8_t c) { return (c >= '0' && c <= '9') || c == '_'; };
    int64_t p = n;
    while (p > 0 && digit(s[p - 1])) --p;
    if (p == n || p == 0) return false;
    if (s[p - 1] == ',' || s[p - 1] == '-') p -= 1;
    else if (p >= 2 && s[p - 1] == '.' && s[p - 2] == '.') p -= 2;
    else return false;
    const int64_t e = p;
    while (p > 0 && digit(s[p - 1])) --p;
    return p != e && p >= 2 && s[p - 1] == ':';
}

struct conc_slice {
    int32_t start, len, rev;            // bytes [start, start + len) of the sequence, reversed and complemented where rev
};

// Bio::DB::Fasta::subseq and caloffset on a sequence of L >= 1 bytes
CONC_HD conc_slice conc_subseq(int64_t start2, int64_t stop2, int64_t L)
{
    if (start2 == 0) start2 = 2;                        // $start ||= 1
    if (stop2 == 0) stop2 = 2 * L;                      // $stop ||= length
    int32_t rev = 0;
    if (start2 > stop2) {
        const int64_t t = start2;
        start2 = stop2;
        stop2 = t;
        rev = 1;
    }
    auto offset = [L](int64_t p2) {                     // $a = shift() - 1, clamped, its fraction dropped
        const int64_t a2 = p2 - 2;
        if (a2 < 0) return (int64_t)0;
        if (a2 >= 2 * L) return L - 1;
        return a2 >> 1;
    };
    const int64_t a = offset(start2), b = offset(stop2);
    return conc_slice{(int32_t)a, (int32_t)(b - a + 1), rev};
}

CONC_HD int64_t conc_tx_length(const conc_view& v, int32_t t)
{
    int64_t n = 0;
    for (int32_t k = 0; k < v.tx[t].exon_count; ++k) n += (int64_t)v.exons[v.tx[t].exon_first + k].end - v.exons[v.tx[t].exon_first + k].start + 1;
    return n;
}

// gene_models.pm:372-412 for a transcript t
CONC_HD int64_t conc_genomic_position2(const conc_view& v, int32_t t, int64_t p2)
{
    const conc_transcript T = v.tx[t];
    const conc_interval* ex = v.exons + T.exon_first;
    if (T.strand == 1) p2 = 2 * conc_tx_length(v, t) - p2 + 2;
    if (p2 < 2) return 2 * (int64_t)ex[0].start + p2 - 2;
    int64_t off = 0;
    for (int32_t k = 0; k < T.exon_count; ++k) {
        const int64_t size = (int64_t)ex[k].end - ex[k].start + 1;
        if (p2 <= 2 * (off + size)) return p2 - 2 * off - 2 + 2 * (int64_t)ex[k].start;
        off += size;
    }
    return p2 - 2 * off + 2 * (int64_t)ex[T.exon_count - 1].end;
}

// gene_models.pm:528-570: the position in transcript t of a genomic position
CONC_HD int64_t conc_transcript_position2(const conc_view& v, int32_t t, int64_t p2)
{
    const conc_transcript T = v.tx[t];
    const conc_interval* ex = v.exons + T.exon_first;
    const int64_t L = conc_tx_length(v, t);
    int64_t off = 0, found2 = 2 * L;
    for (int32_t k = 0; k < T.exon_count; ++k) {
        if (p2 <= 2 * (int64_t)ex[k].end) {
            found2 = p2 < 2 * (int64_t)ex[k].start ? 2 * off + 2 : 2 * off + p2 - 2 * (int64_t)ex[k].start + 2;
            break;
        }
        off += (int64_t)ex[k].end - ex[k].start + 1;
    }
    return T.strand == 1 ? 2 * L - found2 + 2 : found2;
}

// calc_gene_location is coding, utr5p or utr3p
CONC_HD bool conc_expressed(const conc_view& v, int32_t g, int64_t p2)
{
    const conc_gene G = v.genes[g];
    if (p2 < 2 * (int64_t)G.start || p2 > 2 * (int64_t)G.end) return false;
    for (int32_t k = 0; k < G.tx_count; ++k) {
        const conc_transcript T = v.tx[v.gene_tx[G.tx_first + k]];
        for (int32_t i = 0; i < T.expr_count; ++i) {
            const conc_interval iv = v.expr[T.expr_first + i];
            if (p2 >= 2 * (int64_t)iv.start && p2 <= 2 * (int64_t)iv.end) return true;
        }
    }
    return false;
}

// does a piece of calc_genomic_regions(t, [s, e]) (gene_models.pm:415-469) overlap [gs, ge]?  least / greatest: the hull of the pieces
CONC_HD bool conc_tx_pieces(const conc_view& v, int32_t t, int64_t s, int64_t e, int64_t gs, int64_t ge, int64_t* least, int64_t* greatest)
{
    const conc_transcript T = v.tx[t];
    const conc_interval* ex = v.exons + T.exon_first;
    const int64_t L = conc_tx_length(v, t);
    int64_t r0 = s, r1 = e;
    if (T.strand == 1) {
        r0 = L - e + 1;
        r1 = L - s + 1;
    }
    if (r0 < 1) r0 = 1;
    if (r1 > L) r1 = L;
    bool hit = false;
    int64_t off = 0;
    for (int32_t k = 0; k < T.exon_count; ++k) {
        const int64_t size = (int64_t)ex[k].end - ex[k].start + 1;
        const int64_t ls = r0 - off, le = r1 - off;
        const int64_t a = (ls > 1 ? ls : 1) + ex[k].start - 1, b = (le < size ? le : size) + ex[k].start - 1;
        if (a <= b) {
            if (least && a < *least) *least = a;
            if (greatest && b > *greatest) *greatest = b;
            if (!(b < gs || a > ge)) hit = true;
        }
        off += size;
    }
    return hit;
}

// calc_overlapping_genes(ref, [s, e]) for a reference that is transcript t (t >= 0) or the known chromosome c: visit(gene) once per
// gene, in the order of the chromosome's list.  The 10 000-base bins of the script only index the genes, except for a region
// with s > e on a chromosome: its bins are int(s / 10000) .. int(e / 10000), none unless both are one bin, which the gene must touch.
template <class Visit>
CONC_HD void conc_overlapping_genes(const conc_view& v, int32_t t, int32_t c, int64_t s, int64_t e, Visit visit)
{
    int64_t lo = s, hi = e;                             // genes with start <= hi and end >= lo are looked at
    if (t >= 0) {
        c = v.tx[t].chrom;
        lo = INT64_MAX;
        hi = INT64_MIN;
        (void)conc_tx_pieces(v, t, s, e, 0, -1, &lo, &hi);
        if (lo > hi) return;
    } else if (s > e && s / 10000 != e / 10000) return;
    const int32_t first = v.chrom_gene_first[c], n = v.chrom_gene_first[c + 1] - first;
    int32_t a = 0, b = n;                               // the genes in front of b start at or below hi
    while (a < b) {
        const int32_t mid = a + (b - a) / 2;
        if ((int64_t)v.genes[v.chrom_genes[first + mid]].start <= hi) a = mid + 1;
        else b = mid;
    }
    int32_t from = b;                                   // walk back while some gene up to there ends at or behind lo
    while (from > 0 && (int64_t)v.chrom_premax[first + from - 1] >= lo) --from;
    for (int32_t k = from; k < b; ++k) {
        const int32_t g = v.chrom_genes[first + k];
        const conc_gene G = v.genes[g];
        bool hit;
        if (t >= 0) hit = conc_tx_pieces(v, t, s, e, G.start, G.end, nullptr, nullptr);
        else {
            hit = !(e < (int64_t)G.start || s > (int64_t)G.end);
            if (hit && s > e) hit = G.start / 10000 <= s / 10000 && s / 10000 <= G.end / 10000;
        }
        if (hit) visit(g);
    }
}

// one end of a cluster as read_clusters leaves it (prep_local_alignment_seqs.pl:158-188)
struct conc_end {
    const uint8_t* name;
    int32_t name_len;
    int32_t strand;                     // 0 "+", 1 "-"
    int32_t start, end;
};

// what both passes (count, emit) of an end share
struct conc_end_plan {
    int32_t stop;                       // 0 or CONC_*
    int32_t limit;                      // a DSA_E_LIMIT condition
    int32_t tx, chrom;                  // what the name is in the models, -1 each
    int32_t seq0;                       // the sequence of the genomic target, -1: skipped
    int32_t name0;                      // conc_target.name of the genomic target
    int32_t gstrand;                    // the genomic strand
    int64_t gmid2;
    int32_t other_seq, other_strand;
    conc_slice other;
};

CONC_HD conc_end_plan conc_plan_end(const conc_view& v, const conc_end& me, const conc_end& other)
{
    conc_end_plan P{};
    P.tx = P.chrom = P.seq0 = P.name0 = P.other_seq = -1;
    if (me.name_len == 0 || other.name_len == 0) {
        P.stop = CONC_EMPTY_NAME;
        return P;
    }
    if (conc_name_is_range(me.name, me.name_len) || conc_name_is_range(other.name, other.name_len)) {
        P.limit = 1;
        return P;
    }
    P.other_strand = other.strand;
    P.other_seq = conc_find_name(v.names, v.seq_names, v.seq_sorted, v.n_seqs, other.name, other.name_len);
    if (P.other_seq < 0) {
        P.stop = CONC_NO_OTHER_SEQ;
        return P;
    }
    if (v.seqs[P.other_seq].len < 1) {
        P.stop = CONC_EMPTY_OTHER;
        return P;
    }
    P.other = conc_subseq(2 * (int64_t)other.start, 2 * (int64_t)other.end, v.seqs[P.other_seq].len);
    P.tx = conc_find_name(v.names, v.tx_names, nullptr, v.n_tx, me.name, me.name_len);
    P.chrom = conc_find_name(v.names, v.chrom_names, nullptr, v.n_chroms, me.name, me.name_len);
    const int64_t mid2 = (int64_t)me.start + me.end;
    if (P.tx >= 0) {                                    // a name that is both is a transcript to the three calc_genomic_* functions
        P.name0 = v.tx[P.tx].chrom;
        P.seq0 = v.chrom_seq[P.name0];
        P.gmid2 = conc_genomic_position2(v, P.tx, mid2);
        P.gstrand = v.tx[P.tx].strand == me.strand ? 0 : 1;
    } else {
        P.name0 = P.chrom;
        P.seq0 = conc_find_name(v.names, v.seq_names, v.seq_sorted, v.n_seqs, me.name, me.name_len);
        P.gmid2 = mid2;
        P.gstrand = me.strand;
    }
    return P;
}

// the window of a target at mid2 on `strand` of sequence `seq` (>= 0): false (and limit set) for a sequence without bytes
CONC_HD bool conc_window(const conc_view& v, const conc_end_plan& P, int32_t seq, int64_t mid2, int32_t strand, int64_t range, conc_target& T, int32_t& limit)
{
    const int64_t L = v.seqs[seq].len;
    if (L < 1) {
        limit = 1;
        return false;
    }
    const conc_slice w = strand == 0 ? conc_subseq(mid2, mid2 + 2 * range, L) : conc_subseq(mid2 - 2 * range, mid2, L);
    T.seq = seq;
    T.start = w.start;
    T.len = w.len;
    T.revcomp = w.rev ^ (strand == P.other_strand ? 1 : 0);
    T.other_seq = P.other_seq;
    T.other_start = P.other.start;
    T.other_len = P.other.len;
    T.other_rev = P.other.rev;
    return true;
}

// Every target of one end: emit(target, rank) with rank 0 for the genomic target and 1 + the transcript's place in gene_tx for the
// others (ascending rank is the canonical order within an end).  Returns the number of targets; `limit` is set for DSA_E_LIMIT.
template <class Emit>
CONC_HD int64_t conc_end_targets(const conc_view& v, const conc_end_plan& P, const conc_end& me, int32_t cluster_id, int32_t cluster_end, int64_t range,
                                 int32_t& limit, Emit emit)
{
    int64_t n = 0;
    conc_target T{};
    T.cluster_id = cluster_id;
    T.cluster_end = cluster_end;
    if (P.seq0 >= 0) {
        T.kind = CONC_KIND_GENOMIC;
        T.name = P.name0;
        if (conc_window(v, P, P.seq0, P.gmid2, P.gstrand, range, T, limit)) {
            emit(T, (int64_t)0);
            ++n;
        }
    }
    if (P.tx < 0 && P.chrom < 0) return n;
    conc_overlapping_genes(v, P.tx, P.chrom, me.start, me.end, [&](int32_t g) {
        if (!conc_expressed(v, g, P.gmid2)) return;
        const conc_gene G = v.genes[g];
        for (int32_t k = 0; k < G.tx_count; ++k) {
            const int32_t t = v.gene_tx[G.tx_first + k];
            if (v.tx_seq[t] < 0) continue;
            T.kind = CONC_KIND_TRANSCRIPT;
            T.name = t;
            const int32_t strand = v.tx[t].strand == P.gstrand ? 0 : 1;
            if (conc_window(v, P, v.tx_seq[t], conc_transcript_position2(v, t, P.gmid2), strand, range, T, limit)) {
                emit(T, (int64_t)1 + G.tx_first + k);
                ++n;
            }
        }
    });
    return n;
}
