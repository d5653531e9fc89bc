// taskc_shared.hpp — the rules of one line of a cluster file as remove_duplicates and get_align_regions read it
// (include/defuse_task.h, section "cluster text"), as __host__ __device__ code: the parse kernel of taskc_api.hip and a host
// program (tests/test_cluster_regions.py) compile the same function.
//
// The caller supplies field_int(p, n, v), the integer rule of a field (the device has it beside its tables, the host in
// tools_src/defuse_host.hpp).  Every read of the text is inside [s, e).
#pragma once
#include <stdint.h>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_task.h"

#if defined(__HIPCC__)
#define TASKC_HD __host__ __device__ inline
#else
#define TASKC_HD inline
#endif

// One line, read once for both steps.  Offsets are relative to the line's first byte (a line has fewer than 2^31 bytes).
struct taskc_line {
    int32_t id, ce, frag;       // fields 0, 1, 2 where they are integers, else 0
    int32_t pos;                // dedup: field 6 on a "+" line, else field 7 (dkind 0 and ce 0 / 1 only)
    int32_t start, end;         // regions: fields 6 and 7 (rkind 0 only)
    int32_t name_off, name_len; // field 4
    int32_t strand_off, strand_len;   // field 5
    uint8_t dkind, rkind;       // 0 or TASKC_FEW_FIELDS / TASKC_BAD_INTEGER, by the rules of either step
    int8_t dfield, rfield;      // the field that stopped, else -1
};

template <class FieldInt>
TASKC_HD taskc_line taskc_parse_line(const uint8_t* text, int64_t s, int64_t e, FieldInt field_int)
{
    taskc_line L{};
    L.dfield = L.rfield = -1;
    // field k is text[from[k], to[k]): field 7 ends at the eighth tab or at the line's end
    int64_t from[8], to[8];
    int n = 0;
    from[0] = s;
    for (int64_t p = s; p < e && n < 8; ++p)
        if (text[p] == '\t') {
            to[n++] = p;
            if (n < 8) from[n] = p + 1;
        }
    if (n < 8) to[n++] = e;
    if (n < 8) {
        L.dkind = L.rkind = TASKC_FEW_FIELDS;
        return L;
    }
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool ok[8];
    for (int k = 0; k < 8; ++k) ok[k] = (k <= 2 || k >= 6) && field_int(text + from[k], to[k] - from[k], v[k]);
    L.id = ok[0] ? v[0] : 0;
    L.ce = ok[1] ? v[1] : 0;
    L.frag = ok[2] ? v[2] : 0;
    L.name_off = (int32_t)(from[4] - s);
    L.name_len = (int32_t)(to[4] - from[4]);
    L.strand_off = (int32_t)(from[5] - s);
    L.strand_len = (int32_t)(to[5] - from[5]);
    // remove_duplicates: fields 0, 1, 2; a cluster end other than 0 / 1 ends the look at the line; then the position field
    const int first3 = !ok[0] ? 0 : !ok[1] ? 1 : !ok[2] ? 2 : -1;
    if (first3 >= 0) {
        L.dkind = TASKC_BAD_INTEGER;
        L.dfield = (int8_t)first3;
    } else if (v[1] == 0 || v[1] == 1) {
        const int pf = (L.strand_len == 1 && text[from[5]] == '+') ? 6 : 7;
        if (!ok[pf]) {
            L.dkind = TASKC_BAD_INTEGER;
            L.dfield = (int8_t)pf;
        } else L.pos = v[pf];
    }
    // get_align_regions: fields 0, 1, 6, 7
    const int first4 = !ok[0] ? 0 : !ok[1] ? 1 : !ok[6] ? 6 : !ok[7] ? 7 : -1;
    if (first4 >= 0) {
        L.rkind = TASKC_BAD_INTEGER;
        L.rfield = (int8_t)first4;
    } else {
        L.start = v[6];
        L.end = v[7];
    }
    return L;
}

// What a later step on the same device reads of a taskc_ctx in place (taskc_api.hip: taskc_lines_device; span_api.hip): the
// text, every input line's start and length, its parsed record, and the lines of the source - item k of the source is input
// line src[k], or k itself where src is null.  Device pointers, valid until the next call on the taskc_ctx.
struct taskc_lines_view {
    int device;
    const uint8_t* text;
    const int64_t* lstart;
    const int32_t* llen;
    const taskc_line* rec;
    const uint32_t* src;
    int64_t n_input_lines, n_lines;
};

// The groups of taskc_regions over the input (taskc_api.hip: taskc_groups_device; conc_api.hip).
struct taskc_groups_view {
    const unsigned long long* key;      // ((id ^ sign bit) << 32) | (end ^ sign bit), ascending
    const int32_t* gmin;
    const int32_t* gmax;
    const uint32_t* glast;
    int64_t n_groups;
};

// bytes of v in plain decimal
TASKC_HD int taskc_dec_len(int32_t v)
{
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    int n = v < 0 ? 2 : 1;
    while (u >= 10u) {
        u /= 10u;
        ++n;
    }
    return n;
}

// writes them at out, returns their number
TASKC_HD int taskc_dec_put(int32_t v, uint8_t* out)
{
    const int n = taskc_dec_len(v);
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    for (int k = n - 1; k >= (v < 0 ? 1 : 0); --k) {
        out[k] = (uint8_t)('0' + u % 10u);
        u /= 10u;
    }
    if (v < 0) out[0] = '-';
    return n;
}
