// task_check.hpp — what task_api.hip does before it touches a device: the argument and limit checks of include/defuse_task.h
// and the exon table's derived columns (transcript lengths, regions, the bins of ExonRegions::Read).  Plain host C++ without
// HIP, so that a host program under a sanitizer compiles the same functions (tests/test_task_store.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/defuse_task.h"

namespace taskhost {

inline int fail(std::string& sink, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int fail(std::string& sink, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    sink = buf;
    return code;
}

inline bool coord_ok(int32_t x) { return x >= -TASK_MAX_COORD && x <= TASK_MAX_COORD; }

inline int check_reference(const uint8_t* bytes, int64_t bytes_len, const task_seq* seqs, int64_t n, std::string& err)
{
    if (n < 0 || bytes_len < 0) return fail(err, DSA_E_ARG, "negative size (%lld sequences, %lld bytes)", (long long)n, (long long)bytes_len);
    if (n > (int64_t)INT32_MAX) return fail(err, DSA_E_LIMIT, "more than 2^31 - 1 sequences in one reference");
    if ((n && !seqs) || (bytes_len && !bytes)) return fail(err, DSA_E_ARG, "task_reference_create: null pointer with non-zero size");
    for (int64_t s = 0; s < n; ++s) {
        if (seqs[s].len < 0 || seqs[s].off < 0 || seqs[s].off > bytes_len || seqs[s].len > bytes_len - seqs[s].off)
            return fail(err, DSA_E_ARG, "sequence %lld: bytes %lld + %lld are outside the %lld given", (long long)s, (long long)seqs[s].off,
                        (long long)seqs[s].len, (long long)bytes_len);
        if (seqs[s].len > (int64_t)TASK_MAX_SEQ_LEN) return fail(err, DSA_E_LIMIT, "sequence %lld: longer than %d bytes", (long long)s, TASK_MAX_SEQ_LEN);
    }
    return DSA_OK;
}

// The derived columns of an exon table.  Bins as ExonRegions::Read enters them (tools/ExonRegions.cpp:96-100): a transcript is
// in bins start / 100000 ... end / 100000 of its chromosome with C++ int division, in none if the first is above the last.
// Per chromosome the bins from its lowest to its highest are rows of one CSR; a row lists its transcripts ascending.
struct ExonIndex {
    std::vector<int32_t> tx_len;            // per transcript: the sum of its exons' lengths
    std::vector<int32_t> tx_reg;            // per transcript: first exon's start, last exon's end
    std::vector<int32_t> chrom_bin_lo;      // per chromosome: its lowest bin
    std::vector<int32_t> chrom_bins;        // per chromosome: its number of rows, 0: "invalid chromosome"
    std::vector<int32_t> chrom_row;         // per chromosome: its first row
    std::vector<int32_t> row_first;         // rows + 1
    std::vector<int32_t> row_tx;
};

inline int build_exons(const int32_t* chrom_ref, int32_t n_chroms, const task_transcript* tx, int32_t n_tx, const task_exon* exons, int64_t n_exons,
                       ExonIndex& out, std::string& err)
{
    if (n_chroms < 0 || n_tx < 0 || n_exons < 0)
        return fail(err, DSA_E_ARG, "negative size (%d chromosomes, %d transcripts, %lld exons)", n_chroms, n_tx, (long long)n_exons);
    if (n_exons > (int64_t)INT32_MAX) return fail(err, DSA_E_LIMIT, "more than 2^31 - 1 exons in one table");
    if ((n_chroms && !chrom_ref) || (n_tx && !tx) || (n_exons && !exons)) return fail(err, DSA_E_ARG, "task_exons_create: null pointer with non-zero size");
    for (int32_t c = 0; c < n_chroms; ++c)
        if (chrom_ref[c] < 0) return fail(err, DSA_E_ARG, "chromosome %d: negative reference index %d", c, chrom_ref[c]);
    out = ExonIndex();
    out.tx_len.resize((size_t)n_tx);
    out.tx_reg.resize(2 * (size_t)n_tx);
    out.chrom_bin_lo.assign((size_t)n_chroms, INT32_MAX);
    std::vector<int32_t> hi((size_t)n_chroms, INT32_MIN);
    for (int32_t t = 0; t < n_tx; ++t) {
        const task_transcript& x = tx[t];
        if (x.n_exons < 1) return fail(err, DSA_E_ARG, "transcript %d: no exons (n_exons %d)", t, x.n_exons);
        if (x.first_exon < 0 || (int64_t)x.first_exon + x.n_exons > n_exons)
            return fail(err, DSA_E_ARG, "transcript %d: exons %d + %d are outside the %lld given", t, x.first_exon, x.n_exons, (long long)n_exons);
        if (x.chrom < 0 || x.chrom >= n_chroms) return fail(err, DSA_E_ARG, "transcript %d: chromosome %d is not one of %d", t, x.chrom, n_chroms);
        if (x.strand != 0 && x.strand != 1) return fail(err, DSA_E_ARG, "transcript %d: strand %d is not 0 or 1", t, x.strand);
        if (x.name_ref < 0) return fail(err, DSA_E_ARG, "transcript %d: negative name_ref %d", t, x.name_ref);
        int64_t len = 0, span = 0;
        for (int32_t k = 0; k < x.n_exons; ++k) {
            const task_exon& e = exons[x.first_exon + k];
            if (!coord_ok(e.start) || !coord_ok(e.end))
                return fail(err, DSA_E_LIMIT, "transcript %d: exon %d (%d, %d) has a coordinate beyond +-%d", t, k, e.start, e.end, TASK_MAX_COORD);
            const int64_t n = (int64_t)e.end - e.start + 1;
            len += n;
            span += n < 0 ? -n : n;
        }
        if (span > (int64_t)TASK_MAX_COORD) return fail(err, DSA_E_LIMIT, "transcript %d: its exons cover more than %d bases", t, TASK_MAX_COORD);
        out.tx_len[(size_t)t] = (int32_t)len;
        const int32_t r0 = exons[x.first_exon].start, r1 = exons[x.first_exon + x.n_exons - 1].end;
        out.tx_reg[2 * (size_t)t] = r0;
        out.tx_reg[2 * (size_t)t + 1] = r1;
        const int32_t b0 = r0 / TASK_EXON_BIN, b1 = r1 / TASK_EXON_BIN;
        if (b0 <= b1) {
            out.chrom_bin_lo[(size_t)x.chrom] = std::min(out.chrom_bin_lo[(size_t)x.chrom], b0);
            hi[(size_t)x.chrom] = std::max(hi[(size_t)x.chrom], b1);
        }
    }
    out.chrom_bins.resize((size_t)n_chroms);
    out.chrom_row.resize((size_t)n_chroms);
    int64_t rows = 0;
    for (int32_t c = 0; c < n_chroms; ++c) {
        const bool any = hi[(size_t)c] >= out.chrom_bin_lo[(size_t)c];
        if (!any) out.chrom_bin_lo[(size_t)c] = 0;
        out.chrom_bins[(size_t)c] = any ? hi[(size_t)c] - out.chrom_bin_lo[(size_t)c] + 1 : 0;
        out.chrom_row[(size_t)c] = (int32_t)rows;
        rows += out.chrom_bins[(size_t)c];
        if (rows > (int64_t)INT32_MAX / 2) return fail(err, DSA_E_LIMIT, "chromosome %d: more than 2^30 bins of %d in one table", c, TASK_EXON_BIN);
    }
    // rows of the CSR: count, sum, fill in transcript order (so every row is ascending)
    out.row_first.assign((size_t)rows + 1, 0);
    int64_t entries = 0;
    for (int32_t t = 0; t < n_tx; ++t) {
        const int32_t b0 = out.tx_reg[2 * (size_t)t] / TASK_EXON_BIN, b1 = out.tx_reg[2 * (size_t)t + 1] / TASK_EXON_BIN;
        const int32_t c = tx[t].chrom;
        for (int32_t b = b0; b <= b1; ++b) ++out.row_first[(size_t)(out.chrom_row[(size_t)c] + (b - out.chrom_bin_lo[(size_t)c])) + 1];
        if (b0 <= b1) entries += b1 - b0 + 1;
        if (entries > (int64_t)INT32_MAX) return fail(err, DSA_E_LIMIT, "transcript %d: more than 2^31 - 1 (transcript, bin) entries in one table", t);
    }
    for (int64_t r = 0; r < rows; ++r) out.row_first[(size_t)r + 1] += out.row_first[(size_t)r];
    out.row_tx.resize((size_t)entries);
    std::vector<int32_t> cursor(out.row_first.begin(), out.row_first.end() - 1);
    for (int32_t t = 0; t < n_tx; ++t) {
        const int32_t b0 = out.tx_reg[2 * (size_t)t] / TASK_EXON_BIN, b1 = out.tx_reg[2 * (size_t)t + 1] / TASK_EXON_BIN;
        const int32_t c = tx[t].chrom;
        for (int32_t b = b0; b <= b1; ++b) out.row_tx[(size_t)cursor[(size_t)(out.chrom_row[(size_t)c] + (b - out.chrom_bin_lo[(size_t)c]))]++] = t;
    }
    return DSA_OK;
}

inline int check_params(const task_params* p, std::string& err)
{
    if (!p) return fail(err, DSA_E_ARG, "task_store_create: no params");
    if (p->min_read < 0 || p->max_read < 0) return fail(err, DSA_E_ARG, "params: negative read length (min_read %d, max_read %d)", p->min_read, p->max_read);
    if (p->min_read > TASK_MAX_PARAM || p->max_read > TASK_MAX_PARAM || p->min_fragment < -TASK_MAX_PARAM || p->min_fragment > TASK_MAX_PARAM ||
        p->max_fragment < -TASK_MAX_PARAM || p->max_fragment > TASK_MAX_PARAM)
        return fail(err, DSA_E_LIMIT, "params: (%d, %d, %d, %d) has a value beyond +-%d", p->min_fragment, p->max_fragment, p->min_read, p->max_read,
                    TASK_MAX_PARAM);
    return DSA_OK;
}

// what can be told from the pairs alone
inline int check_pairs(const task_pair* pairs, int64_t n, std::string& err)
{
    if (n < 0) return fail(err, DSA_E_ARG, "negative number of pairs (%lld)", (long long)n);
    if (n > (int64_t)INT32_MAX / 2) return fail(err, DSA_E_LIMIT, "more than 2^30 - 1 pairs in one store");
    if (n && !pairs) return fail(err, DSA_E_ARG, "task_store_create: null pointer with non-zero size");
    bool ascending = true;
    for (int64_t k = 0; k < n; ++k) {
        const task_pair& p = pairs[k];
        if (p.fusion_id < 0) return fail(err, DSA_E_ARG, "pair %lld: fusion_id %d is outside [0, 2^31)", (long long)k, p.fusion_id);
        if (k && p.fusion_id <= pairs[k - 1].fusion_id) ascending = false;
        for (int e = 0; e < 2; ++e) {
            const task_end& a = p.end[e];
            if (a.strand != 0 && a.strand != 1) return fail(err, DSA_E_ARG, "pair %lld: end[%d].strand %d is not 0 or 1", (long long)k, e, a.strand);
            if (a.seq < -1 || a.transcript < -1 || a.chrom < -1)
                return fail(err, DSA_E_ARG, "pair %lld: end[%d] has an index below -1 (seq %d, transcript %d, chrom %d)", (long long)k, e, a.seq, a.transcript,
                            a.chrom);
            if (!coord_ok(a.start) || !coord_ok(a.end))
                return fail(err, DSA_E_LIMIT, "pair %lld: end[%d] (%d, %d) has a coordinate beyond +-%d", (long long)k, e, a.start, a.end, TASK_MAX_COORD);
            const int64_t len = (int64_t)a.end - a.start + 1;
            if (len > TASK_MAX_REGION || len < -TASK_MAX_REGION)
                return fail(err, DSA_E_LIMIT, "pair %lld: end[%d] (%d, %d) spans more than %d bases", (long long)k, e, a.start, a.end, TASK_MAX_REGION);
        }
    }
    if (!ascending) {           // (the ids of a regions file come ascending: the sort is the other callers')
        std::vector<std::pair<int32_t, int64_t>> byid((size_t)n);
        for (int64_t k = 0; k < n; ++k) byid[(size_t)k] = {pairs[k].fusion_id, k};
        std::sort(byid.begin(), byid.end());
        for (int64_t s = 1; s < n; ++s)
            if (byid[(size_t)s].first == byid[(size_t)s - 1].first)
                return fail(err, DSA_E_ARG, "pairs %lld and %lld: both have fusion_id %d", (long long)byid[(size_t)s - 1].second, (long long)byid[(size_t)s].second,
                            byid[(size_t)s].first);
    }
    return DSA_OK;
}

// the indices of the pairs against the sizes of the two tables
inline int check_pair_indices(const task_pair* pairs, int64_t n, int64_t n_seqs, int32_t n_tx, int32_t n_chroms, std::string& err)
{
    for (int64_t k = 0; k < n; ++k)
        for (int e = 0; e < 2; ++e) {
            const task_end& a = pairs[k].end[e];
            if (a.seq >= n_seqs) return fail(err, DSA_E_ARG, "pair %lld: end[%d].seq %d is not one of %lld sequences", (long long)k, e, a.seq, (long long)n_seqs);
            if (a.transcript >= n_tx) return fail(err, DSA_E_ARG, "pair %lld: end[%d].transcript %d is not one of %d transcripts", (long long)k, e, a.transcript, n_tx);
            if (a.chrom >= n_chroms) return fail(err, DSA_E_ARG, "pair %lld: end[%d].chrom %d is not one of %d chromosomes", (long long)k, e, a.chrom, n_chroms);
        }
    return DSA_OK;
}

}  // namespace taskhost
