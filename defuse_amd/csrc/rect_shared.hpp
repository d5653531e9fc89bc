// rect_shared.hpp — the rule of one line of an alignment file (include/defuse_rec.h, section "alignment text"), as
// __host__ __device__ code: the kernels of rect_api.hip and a host program (tests/test_rectext.py) compile the same function.
// It is the reading side of rec_shared.hpp: field bounds in, the record, the stop and whether the line is plain out.
//
// The caller supplies two things the two sides have in different forms:
//   tab(k)              the position of the line's k-th tab, k < n_tabs (the device reads its tab table, a host program scans);
//   field_int(p, n, v)  the integer rule of a field (the device has it beside its tables, the host in tools_src/defuse_host.hpp).
#pragma once
#include <stdint.h>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_rec.h"
#include "rec_shared.hpp"

struct rect_line {
    dsa_record rec;             // valid if kind == 0
    int32_t kind;               // 0, or RECT_FEW_FIELDS ...
    int32_t field;              // the field that stopped; -1 for RECT_FEW_FIELDS and without a stop
    int32_t id_read, id;        // at least seven fields and field 0 an integer; that integer
    int32_t plain;              // kind == 0 and the bytes are what rec_write_line prints for rec (without the newline)
};

// A field's text is what "%d" prints for the value it parsed to iff it is as short as that: a '+', a leading zero and "-0"
// each add a byte, and nothing but sign and digits has parsed.
REC_HD bool rect_canonical(int32_t v, int64_t n) { return n == (int64_t)(rec_digits(rec_magnitude(v)) + (v < 0 ? 1 : 0)); }

// The line text[s, e) (no newline) with n_tabs tabs.  Only the first nine tabs are looked at.
template <class Tab, class FieldInt>
REC_HD rect_line rect_parse_line(const uint8_t* text, int64_t s, int64_t e, int64_t n_tabs, Tab tab, FieldInt field_int)
{
    rect_line L{};
    L.field = -1;
    int32_t* out = reinterpret_cast<int32_t*>(&L.rec);
    if (n_tabs >= 6) {                                            // seven fields: what the reference's look-ahead asks for
        int id = 0;
        if (field_int(text + s, tab(0) - s, id)) {
            L.id_read = 1;
            L.id = id;
        }
    }
    if (n_tabs < REC_FIELDS - 1) {
        L.kind = RECT_FEW_FIELDS;
        return L;
    }
    bool canonical = true;
    int64_t from = s;
    for (int k = 0; k < REC_FIELDS; ++k) {
        const int64_t to = k < n_tabs ? tab(k) : e;               // (the ninth field of a line with eight tabs ends the line)
        const int64_t n = to - from;
        int v = 0;
        if (k == 3) {
            if (n != 1 || (text[from] != '0' && text[from] != '1')) {
                L.kind = RECT_BAD_BOOL;
                L.field = k;
                return L;
            }
            v = text[from] - '0';
        } else if (!field_int(text + from, n, v)) {
            L.kind = RECT_BAD_INTEGER;
            L.field = k;
            return L;
        } else {
            canonical = canonical && rect_canonical(v, n);
        }
        out[k] = v;
        from = to + 1;
    }
    // nine canonical fields, each closed by a tab, and nothing behind the ninth tab
    L.plain = (canonical && n_tabs == REC_FIELDS && tab(REC_FIELDS - 1) == e - 1) ? 1 : 0;
    return L;
}
