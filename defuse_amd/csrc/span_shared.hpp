// span_shared.hpp — the rules of splitreads.span.stats (include/defuse_ptext.h, section "span statistics") as __host__ __device__
// code: the kernels of span_api.hip and a host program (tests/test_span_stats.py) compile the same functions.
//
// Lines.  A .break line gives (id, end) -> field 4, a .seq line id -> field 2; a cluster line is read through its taskc_line
// (taskc_shared.hpp), and the one position field its group's strand selects is read from the text again, by itself.  The caller
// supplies field_int(p, n, v), the integer rule of a field, and for the two small files tab(k), the position of a line's k-th tab.
// Every read of a text is inside the line [s, e).
//
// "%.15g".  ptext_shared.hpp's scheme with fifteen digits in 64 bits: |x| is exactly a 64-bit integer part and 128 fraction bits,
// the digits come off by divisions by 10 and multiplications of the limbs by 10, what is left after the fifteenth digit is the
// rounding digit and a sticky bit, so a tie is seen exactly (half-to-even); exponent form if the decimal exponent after rounding
// is < -4 or >= 15; trailing zeros and a bare point stripped; an exponent of at least two digits.  span_g_of takes +-0 and
// 2^-64 <= |x| < 2^64 and declines the rest.
#pragma once
#include <stdint.h>

#include "../../include/defuse_ptext.h"
#include "ptext_shared.hpp"
#include "taskc_shared.hpp"

#define SPAN_HD REC_HD

constexpr int SPAN_G_MAX = 21;                       // "-1.23456789012345e+15", "-0.000123456789012345"
constexpr uint64_t SPAN_E15 = 1000000000000000ull;

// ---------------------------------------------------------------------------------------------- "%.15g"
struct span_g {
    uint64_t digits;            // the fifteen significant digits after rounding, 10^14 .. 10^15 - 1; 0 for +-0
    int32_t exp10;              // the decimal exponent of the first of them
    int32_t neg;                // the sign bit
    int32_t ok;                 // 0: not taken (NaN, an infinity, a denormal, |x| < 2^-64 or >= 2^64)
    int32_t pad_;
};

SPAN_HD span_g span_g_of(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    span_g r{0u, 0, (int32_t)(b >> 63), 0, 0};
    const int be = (int)((b >> 52) & 0x7FFu);
    const uint64_t frac = b & ((1ull << 52) - 1u);
    if (be == 0 && frac == 0) {                                                    // +-0
        r.ok = 1;
        return r;
    }
    const int e2 = be - 1023;
    if (be == 0 || e2 < -64 || e2 > 63) return r;
    const uint64_t m = frac | (1ull << 52);
    const int s = e2 - 52;                                                         // |x| = m * 2^s, -116 <= s <= 11
    uint64_t I, fhi = 0, flo = 0;                                                  // |x| = I + (fhi * 2^64 + flo) / 2^128
    if (s >= 0) {
        I = m << s;
    } else {
        I = -s < 64 ? m >> -s : 0u;
        const int t = 128 + s;                                                     // 12 <= t <= 127
        if (t >= 64) {
            fhi = m << (t - 64);
        } else {
            fhi = m >> (64 - t);
            flo = m << t;
        }
    }
    uint32_t f0 = (uint32_t)(fhi >> 32), f1 = (uint32_t)fhi, f2 = (uint32_t)(flo >> 32), f3 = (uint32_t)flo;
    uint64_t M;
    uint32_t round = 0;
    bool sticky = false;
    int e10;
    if (I >= SPAN_E15) {                                                           // sixteen digits or more before the point
        e10 = 14;
        while (I >= SPAN_E15) {                                                    // at most five times
            const uint64_t q = I / 10u;
            sticky = sticky || round != 0;
            round = (uint32_t)(I - q * 10u);
            I = q;
            ++e10;
        }
        M = I;
        sticky = sticky || (f0 | f1 | f2 | f3) != 0;
    } else {
        M = I;
        int nd = M ? rec_digits64(M) : 0;
        e10 = nd - 1;
        for (int k = 0; k < 40 && nd < 15; ++k) {                                  // at most 19 zeros after the point, then fifteen digits
            const uint32_t d = ptext_mul10(f0, f1, f2, f3);
            if (M == 0 && d == 0) {
                --e10;
            } else {
                M = M * 10u + d;
                ++nd;
            }
        }
        if (nd < 15) return r;                                                     // (never, for the values let in above)
        round = ptext_mul10(f0, f1, f2, f3);
        sticky = (f0 | f1 | f2 | f3) != 0;
    }
    if (round > 5 || (round == 5 && (sticky || (M & 1u)))) {
        if (++M == SPAN_E15) {
            M = SPAN_E15 / 10u;
            ++e10;
        }
    }
    r.digits = M;
    r.exp10 = e10;
    r.ok = 1;
    return r;
}

// the digits without their trailing zeros, and how many are left (1..15); digits != 0
SPAN_HD int span_g_strip(uint64_t& m)
{
    int kept = 15;
    for (uint64_t q = m / 10u; kept > 1 && q * 10u == m; q = m / 10u) {
        m = q;
        --kept;
    }
    return kept;
}

// bytes of the text, 1..SPAN_G_MAX; 0 for a value that is not taken
SPAN_HD int span_g_length(const span_g& g)
{
    if (!g.ok) return 0;
    if (g.digits == 0) return g.neg + 1;
    uint64_t m = g.digits;
    const int kept = span_g_strip(m), e = g.exp10;
    if (e < -4 || e >= 15) return g.neg + kept + (kept > 1 ? 1 : 0) + 4;           // d[.dddd]e+XX
    if (e >= 0) return g.neg + (kept > e + 1 ? kept + 1 : e + 1);
    return g.neg + 1 - e + kept;                                                   // "0." and -e - 1 zeros
}

// the text at out (room for span_g_length(g) bytes, no terminator); returns its length
template <typename Char>
SPAN_HD int span_g_write(const span_g& g, Char* out)
{
    if (!g.ok) return 0;
    int p = 0;
    if (g.neg) out[p++] = '-';
    if (g.digits == 0) {
        out[p++] = '0';
        return p;
    }
    uint64_t m = g.digits;
    int kept = span_g_strip(m);
    const int e = g.exp10;
    if (e < -4 || e >= 15) {
        for (int k = kept - 1; k >= 1; --k) {
            const uint64_t q = m / 10u;
            out[p + 1 + k] = (Char)('0' + (int)(m - q * 10u));
            m = q;
        }
        out[p] = (Char)('0' + (int)m);
        if (kept > 1) out[p + 1] = '.';
        p += kept + (kept > 1 ? 1 : 0);
        const uint32_t a = (uint32_t)(e < 0 ? -e : e);                             // at most 20
        out[p++] = 'e';
        out[p++] = e < 0 ? '-' : '+';
        out[p++] = (Char)('0' + a / 10u);
        out[p++] = (Char)('0' + a % 10u);
        return p;
    }
    if (e >= 0) {
        const int before = e + 1;
        for (; kept < before; ++kept) m *= 10u;                                    // zeros before the point are digits of the text
        for (int k = kept - 1; k >= 0; --k) {
            const uint64_t q = m / 10u;
            out[p + k + (k >= before ? 1 : 0)] = (Char)('0' + (int)(m - q * 10u));
            m = q;
        }
        if (kept > before) out[p + before] = '.';
        return p + kept + (kept > before ? 1 : 0);
    }
    out[p++] = '0';
    out[p++] = '.';
    for (int z = -e - 1; z > 0; --z) out[p++] = '0';
    for (int k = kept - 1; k >= 0; --k) {
        const uint64_t q = m / 10u;
        out[p + k] = (Char)('0' + (int)(m - q * 10u));
        m = q;
    }
    return p + kept;
}

// ---------------------------------------------------------------------------------------------- the lines

// A key field (an id, a cluster end, a fragment): an integer, and whether its bytes are the "%d" of its value ("+7", "007"
// and "-0" are not): Perl keys its hashes by the bytes, the library by the value.
template <class FieldInt>
SPAN_HD bool span_key_field(const uint8_t* p, int64_t n, FieldInt field_int, int32_t& v, int32_t& noncanonical)
{
    int x = 0;
    if (!field_int(p, n, x)) return false;
    v = x;
    uint8_t buf[12];
    const int len = taskc_dec_put(x, buf);
    bool same = (int64_t)len == n;
    for (int k = 0; same && k < len; ++k) same = buf[k] == p[k];
    if (!same) ++noncanonical;
    return true;
}

// one line of the .break or the .seq file
struct span_entry {
    int32_t id, end, value;     // .break: fields 0, 1, 4; .seq: fields 0 and 2, end 0
    int32_t kind, field;        // 0 and -1, or SPAN_FEW_FIELDS / SPAN_BAD_INTEGER and the field
    int32_t noncanonical;       // key fields that are not their "%d"
};

// text[s, e) with n_tabs tabs at tab(0) < tab(1) < ...
template <class Tabs, class FieldInt>
SPAN_HD span_entry span_break_line(const uint8_t* text, int64_t s, int64_t e, Tabs tab, int64_t n_tabs, FieldInt field_int)
{
    span_entry r{0, 0, 0, 0, -1, 0};
    if (n_tabs < 4) {
        r.kind = SPAN_FEW_FIELDS;
        return r;
    }
    const int64_t t0 = tab(0), t1 = tab(1), t3 = tab(3), t4 = n_tabs > 4 ? tab(4) : e;
    int v = 0;
    if (!span_key_field(text + s, t0 - s, field_int, r.id, r.noncanonical)) r.field = 0;
    else if (!span_key_field(text + t0 + 1, t1 - t0 - 1, field_int, r.end, r.noncanonical)) r.field = 1;
    else if (!field_int(text + t3 + 1, t4 - t3 - 1, v)) r.field = 4;
    else r.value = v;
    if (r.field >= 0) r.kind = SPAN_BAD_INTEGER;
    return r;
}

template <class Tabs, class FieldInt>
SPAN_HD span_entry span_seq_line(const uint8_t* text, int64_t s, int64_t e, Tabs tab, int64_t n_tabs, FieldInt field_int)
{
    span_entry r{0, 0, 0, 0, -1, 0};
    if (n_tabs < 2) {
        r.kind = SPAN_FEW_FIELDS;
        return r;
    }
    const int64_t t0 = tab(0), t1 = tab(1), t2 = n_tabs > 2 ? tab(2) : e;
    int v = 0;
    if (!span_key_field(text + s, t0 - s, field_int, r.id, r.noncanonical)) r.field = 0;
    else if (!field_int(text + t1 + 1, t2 - t1 - 1, v)) r.field = 2;
    else r.value = v;
    if (r.field >= 0) r.kind = SPAN_BAD_INTEGER;
    return r;
}

// a cluster line by this step's rule, from its taskc_line: eight fields, and fields 0, 1 and 2 integers
SPAN_HD int span_cluster_stop(const taskc_line& r, int& field)
{
    field = -1;
    if (r.dkind == TASKC_FEW_FIELDS) return SPAN_FEW_FIELDS;
    if (r.dkind == TASKC_BAD_INTEGER && r.dfield <= 2) {
        field = r.dfield;
        return SPAN_BAD_INTEGER;
    }
    return 0;
}

// how many of fields 0, 1, 2 of a cluster line without a stop are not their "%d"
template <class FieldInt>
SPAN_HD int32_t span_cluster_noncanonical(const uint8_t* text, int64_t s, int64_t e, FieldInt field_int)
{
    int32_t n = 0, v = 0;
    int64_t a = s;
    for (int k = 0; k < 3 && a <= e; ++k) {
        int64_t b = a;
        while (b < e && text[b] != '\t') ++b;
        (void)span_key_field(text + a, b - a, field_int, v, n);
        a = b + 1;
    }
    return n;
}

SPAN_HD bool span_is_plus(const taskc_line& r, const uint8_t* text, int64_t s) { return r.strand_len == 1 && text[s + r.strand_off] == '+'; }

// The one position field of a cluster line [s, e) without a stop that a strand selects: field 6 on a plus end, else field 7.
// The other one is not looked at.
template <class FieldInt>
SPAN_HD bool span_position(const uint8_t* text, int64_t s, int64_t e, const taskc_line& r, bool plus, FieldInt field_int, int32_t& v, int32_t& field)
{
    field = plus ? 6 : 7;
    int64_t a = s + r.strand_off + r.strand_len + 1, b = a;                        // field 6, behind the strand's tab
    while (b < e && text[b] != '\t') ++b;
    if (!plus) {
        if (b >= e) return false;                                                  // (never: the line has eight fields)
        a = b + 1;
        for (b = a; b < e && text[b] != '\t';) ++b;
    }
    int x = 0;
    if (a > e || !field_int(text + a, b - a, x)) return false;
    v = x;
    return true;
}

// ---------------------------------------------------------------------------------------------- the numbers
SPAN_HD bool span_coord_ok(int32_t v) { return v >= -TASK_MAX_COORD && v <= TASK_MAX_COORD; }
// what one end of a fragment adds to the fragment's length
SPAN_HD int64_t span_term(bool plus, int32_t break_pos, int32_t pos) { return plus ? (int64_t)break_pos - pos + 1 : (int64_t)pos - break_pos + 1; }
// inside this bound a double holds the sum and Perl's quotient is the one IEEE division
SPAN_HD bool span_sum_ok(int64_t sum) { return sum >= -(1ll << 53) && sum <= (1ll << 53); }
SPAN_HD double span_mean(int64_t sum, int64_t count) { return (double)sum / (double)count; }

// an id's stops in the order they are looked for (the lowest is reported); the value a kernel keeps is 16 * rank + field
SPAN_HD int span_stop_rank(int kind)
{
    return kind == SPAN_NOT_TWO_ENDS ? 1 : kind == SPAN_NO_BREAK_END ? 2 : kind == SPAN_BAD_INTEGER ? 3 : kind == SPAN_COORD_LIMIT ? 4 : kind == SPAN_NO_INTER ? 5 : 6;
}
SPAN_HD int span_stop_kind(int rank)
{
    return rank == 1 ? SPAN_NOT_TWO_ENDS : rank == 2 ? SPAN_NO_BREAK_END : rank == 3 ? SPAN_BAD_INTEGER : rank == 4 ? SPAN_COORD_LIMIT : rank == 5 ? SPAN_NO_INTER : SPAN_SUM_LIMIT;
}

// one row: "%d\t%.15g\t%lld\n"
SPAN_HD int span_row_length(int32_t id, const span_g& mean, int64_t count) { return taskc_dec_len(id) + 1 + span_g_length(mean) + 1 + rec_field_length64(count); }

SPAN_HD int span_row_write(int32_t id, const span_g& mean, int64_t count, uint8_t* out)
{
    int p = taskc_dec_put(id, out);
    out[p++] = '\t';
    p += span_g_write(mean, out + p);
    out[p++] = '\t';
    p += rec_write_field64(count, out + p);
    out[p - 1] = '\n';                                                             // (rec_write_field64 ends a field with a tab)
    return p;
}
