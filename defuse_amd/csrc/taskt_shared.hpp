// taskt_shared.hpp — the rules of one line of the exon table and of the regions file (include/defuse_task.h, section "region
// and exon text"), and the checks of one pair, as __host__ __device__ code: the kernels of taskt_api.hip and a host program
// (tests/test_task_text.py) compile the same functions.
//
// The caller supplies two things the two sides have in different forms:
//   tab(k)              the position of the line's k-th tab, k < n_tabs (the device reads its tab table, a host program scans);
//   field_int(p, n, v)  the integer rule of a field (the device has it beside its tables, the host in tools_src/defuse_host.hpp).
#pragma once
#include <stdint.h>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_task.h"

#if defined(__HIPCC__)
#define TASKT_HD __host__ __device__ inline
#else
#define TASKT_HD inline
#endif

constexpr int32_t TASKT_SKIPPED = -1;         // a line's kind: rule (1)

// field k of the line text[s, e) with n_tabs tabs is text[from, to); k <= n_tabs
template <class Tab>
TASKT_HD void taskt_field(int64_t s, int64_t e, int64_t n_tabs, Tab tab, int64_t k, int64_t& from, int64_t& to)
{
    from = k == 0 ? s : tab(k - 1) + 1;
    to = k < n_tabs ? tab(k) : e;
}

TASKT_HD bool taskt_strand(const uint8_t* text, int64_t from, int64_t to, int32_t& strand)
{
    if (to - from != 1 || (text[from] != '+' && text[from] != '-')) return false;
    strand = text[from] == '+' ? 0 : 1;
    return true;
}

struct taskt_exon_line {
    int32_t kind;               // 0: a transcript, TASKT_SKIPPED, or the stop
    int32_t field;              // the field that stopped, else -1
    int32_t n_exons;            // kind 0: (n_fields - 4) / 2 >= 1
    int32_t strand;             // kind 0
};

// One line of the exon table, without the duplicate rule (which needs the other lines).
template <class Tab, class FieldInt>
TASKT_HD taskt_exon_line taskt_parse_exon_line(const uint8_t* text, int64_t s, int64_t e, int64_t n_tabs, Tab tab, FieldInt field_int)
{
    taskt_exon_line L{0, -1, 0, 0};
    if (e <= s || n_tabs < 5) {
        L.kind = TASKT_SKIPPED;
        return L;
    }
    for (int64_t k = 5; k <= n_tabs; k += 2) {
        for (int64_t j = k - 1; j <= k; ++j) {
            int64_t from, to;
            int v;
            taskt_field(s, e, n_tabs, tab, j, from, to);
            if (!field_int(text + from, to - from, v)) {
                L.kind = TASKT_EXON_BAD_INTEGER;
                L.field = (int32_t)j;
                return L;
            }
        }
        ++L.n_exons;
    }
    int64_t from, to;
    taskt_field(s, e, n_tabs, tab, 3, from, to);
    if (!taskt_strand(text, from, to, L.strand)) {
        L.kind = TASKT_EXON_BAD_STRAND;
        L.field = 3;
        return L;
    }
    for (int k = 1; k <= 2; ++k) {
        taskt_field(s, e, n_tabs, tab, k, from, to);
        if (to - from > TASKT_MAX_NAME) {
            L.kind = TASKT_EXON_LONG_NAME;
            L.field = k;
            return L;
        }
    }
    return L;
}

struct taskt_region_line {
    int32_t kind;               // 0: an end of a pair, TASKT_SKIPPED, or the stop
    int32_t field;              // the field that stopped, else -1
    int32_t id, end;            // kind 0 from here on
    int32_t strand, start, stop;
    int32_t name_len;           // field 2 is text[name_off, name_off + name_len)
    int64_t name_off;
};

template <class Tab, class FieldInt>
TASKT_HD taskt_region_line taskt_parse_region_line(const uint8_t* text, int64_t s, int64_t e, int64_t n_tabs, Tab tab, FieldInt field_int)
{
    taskt_region_line L{};
    L.field = -1;
    if (e <= s || n_tabs < 4) {
        L.kind = TASKT_SKIPPED;
        return L;
    }
    int64_t from, to;
    int v[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        taskt_field(s, e, n_tabs, tab, k, from, to);
        if (!field_int(text + from, to - from, v[k])) {
            L.kind = TASKT_REGION_BAD_INTEGER;
            L.field = k;
            return L;
        }
    }
    if (v[1] != 0 && v[1] != 1) {
        L.kind = TASKT_REGION_BAD_END;
        L.field = 1;
        return L;
    }
    taskt_field(s, e, n_tabs, tab, 3, from, to);
    if (!taskt_strand(text, from, to, L.strand)) {
        L.kind = TASKT_REGION_BAD_STRAND;
        L.field = 3;
        return L;
    }
    int w[2] = {0, 0};
    for (int k = 4; k < 6; ++k) {
        bool ok = n_tabs >= 5;                            // (five fields: field 5 is missing, whatever field 4 holds)
        if (ok) {
            taskt_field(s, e, n_tabs, tab, k, from, to);
            ok = field_int(text + from, to - from, w[k - 4]);
        }
        if (!ok) {
            L.kind = TASKT_REGION_BAD_INTEGER;
            L.field = n_tabs >= 5 ? k : 5;
            return L;
        }
    }
    L.id = v[0];
    L.end = v[1];
    L.start = w[0];
    L.stop = w[1];
    taskt_field(s, e, n_tabs, tab, 2, from, to);
    L.name_off = from;
    L.name_len = (int32_t)(to - from);
    return L;
}

// What taskhost::check_pairs refuses in a pair that the regions parse made (strands and indices are its own): 0, or 1 a
// negative fusion id (DSA_E_ARG), 2 a coordinate beyond TASK_MAX_COORD, 3 a span beyond TASK_MAX_REGION (DSA_E_LIMIT), in
// check_pairs' order; *end is the end of 2 and 3.
TASKT_HD int taskt_pair_fault(const task_pair& p, int* end)
{
    *end = 0;
    if (p.fusion_id < 0) return 1;
    for (int e = 0; e < 2; ++e) {
        const task_end& a = p.end[e];
        *end = e;
        if (a.start < -TASK_MAX_COORD || a.start > TASK_MAX_COORD || a.end < -TASK_MAX_COORD || a.end > TASK_MAX_COORD) return 2;
        const int64_t len = (int64_t)a.end - a.start + 1;
        if (len > TASK_MAX_REGION || len < -TASK_MAX_REGION) return 3;
    }
    return 0;
}
