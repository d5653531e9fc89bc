// ptext_shared.hpp — what the lines of splitreads.seq and splitreads.break are (include/defuse_ptext.h), as __host__ __device__
// code: the kernels of ptext_api.hip and a host program (tests/test_ptext.py) compile the same functions.
//
// "%g".  An ostream prints a double as printf("%g") does: six significant digits, rounded half-to-even on the EXACT binary
// value; exponent form if the decimal exponent after rounding is < -4 or >= 6; trailing zeros and a bare point stripped; an
// exponent of at least two digits.  ptext_g_of takes +-0 and 2^-64 <= |x| < 2^64.  There |x| = m * 2^s with a 53-bit m and
// -116 <= s <= 11, so it is exactly a 64-bit integer part I and 128 fraction bits F, held as four 32-bit limbs.  The digits
// come off I by divisions by the constant 10 and off F by multiplications of the limbs by 10 (the carry out of the top limb
// is the next digit): no wide division, no table, no array that is indexed at run time.  What is left of I and F after the
// sixth digit is the rounding digit and a sticky bit, so a tie is seen exactly.
//
// Integers are printed by rec_shared.hpp's writers.
#pragma once
#include <stdint.h>

#include "../../include/defuse_ptext.h"
#include "rec_shared.hpp"

constexpr int PTEXT_G_MAX = 12;                      // "-0.000123456", "-1.23456e+19"

// a double as "%g" prints it
struct ptext_g {
    uint32_t digits;            // the six significant digits after rounding, 100000 .. 999999; 0 for +-0
    int32_t exp10;              // the decimal exponent of the first of them
    int32_t neg;                // the sign bit
    int32_t ok;                 // 0: not taken (NaN, an infinity, a denormal, |x| < 2^-64 or >= 2^64)
};

// F *= 10 on the four limbs (f0 the most significant); returns the digit carried out
REC_HD uint32_t ptext_mul10(uint32_t& f0, uint32_t& f1, uint32_t& f2, uint32_t& f3)
{
    uint64_t c = (uint64_t)f3 * 10u;
    f3 = (uint32_t)c;
    c = (c >> 32) + (uint64_t)f2 * 10u;
    f2 = (uint32_t)c;
    c = (c >> 32) + (uint64_t)f1 * 10u;
    f1 = (uint32_t)c;
    c = (c >> 32) + (uint64_t)f0 * 10u;
    f0 = (uint32_t)c;
    return (uint32_t)(c >> 32);
}

REC_HD ptext_g ptext_g_of(double x)
{
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    ptext_g r{0u, 0, (int32_t)(b >> 63), 0};
    const int be = (int)((b >> 52) & 0x7FFu);
    const uint64_t frac = b & ((1ull << 52) - 1u);
    if (be == 0 && frac == 0) {                                                    // +-0
        r.ok = 1;
        return r;
    }
    const int e2 = be - 1023;                                                      // 2^e2 <= |x| < 2^(e2 + 1) for a normal x
    if (be == 0 || e2 < -64 || e2 > 63) return r;                                  // (NaN and the infinities have e2 = 1024)
    const uint64_t m = frac | (1ull << 52);
    const int s = e2 - 52;                                                         // |x| = m * 2^s, -116 <= s <= 11
    uint64_t I, fhi = 0, flo = 0;                                                  // |x| = I + (fhi * 2^64 + flo) / 2^128
    if (s >= 0) {
        I = m << s;
    } else {
        I = -s < 64 ? m >> -s : 0u;
        const int t = 128 + s;                                                     // the fraction is m * 2^t mod 2^128, 12 <= t <= 127
        if (t >= 64) {
            fhi = m << (t - 64);                                                   // (the integer bits fall off the top)
        } else {
            fhi = m >> (64 - t);
            flo = m << t;
        }
    }
    uint32_t f0 = (uint32_t)(fhi >> 32), f1 = (uint32_t)fhi, f2 = (uint32_t)(flo >> 32), f3 = (uint32_t)flo;
    uint32_t M, round = 0;
    bool sticky = false;
    int e10;
    if (I >= 1000000u) {                                                           // seven digits or more before the point
        e10 = 5;
        while (I >= 1000000u) {                                                    // at most 14 times
            const uint64_t q = I / 10u;
            sticky = sticky || round != 0;
            round = (uint32_t)(I - q * 10u);
            I = q;
            ++e10;
        }
        M = (uint32_t)I;
        sticky = sticky || (f0 | f1 | f2 | f3) != 0;
    } else {
        M = (uint32_t)I;
        int nd = M ? rec_digits(M) : 0;
        e10 = nd - 1;
        for (int k = 0; k < 25 && nd < 6; ++k) {                                   // at most 19 zeros after the point, then six digits
            const uint32_t d = ptext_mul10(f0, f1, f2, f3);
            if (M == 0 && d == 0) {
                --e10;
            } else {
                M = M * 10u + d;
                ++nd;
            }
        }
        if (nd < 6) return r;                                                      // (never, for the values let in above)
        round = ptext_mul10(f0, f1, f2, f3);
        sticky = (f0 | f1 | f2 | f3) != 0;
    }
    if (round > 5 || (round == 5 && (sticky || (M & 1u)))) {
        if (++M == 1000000u) {
            M = 100000u;
            ++e10;
        }
    }
    r.digits = M;
    r.exp10 = e10;
    r.ok = 1;
    return r;
}

// the digits without their trailing zeros, and how many are left (1..6); digits != 0
REC_HD int ptext_g_strip(uint32_t& m)
{
    int kept = 6;
    for (uint32_t q = m / 10u; kept > 1 && q * 10u == m; q = m / 10u) {
        m = q;
        --kept;
    }
    return kept;
}

// bytes of the text, 1..PTEXT_G_MAX; 0 for a value that is not taken
REC_HD int ptext_g_length(const ptext_g& g)
{
    if (!g.ok) return 0;
    if (g.digits == 0) return g.neg + 1;
    uint32_t m = g.digits;
    const int kept = ptext_g_strip(m), e = g.exp10;
    if (e < -4 || e >= 6) return g.neg + kept + (kept > 1 ? 1 : 0) + 4;            // d[.ddddd]e+XX
    if (e >= 0) return g.neg + (kept > e + 1 ? kept + 1 : e + 1);                  // the e + 1 digits before the point stay
    return g.neg + 1 - e + kept;                                                   // "0." and -e - 1 zeros
}

// the text at out (room for ptext_g_length(g) bytes, no terminator); returns its length
template <typename Char>
REC_HD int ptext_g_write(const ptext_g& g, Char* out)
{
    if (!g.ok) return 0;
    int p = 0;
    if (g.neg) out[p++] = '-';
    if (g.digits == 0) {
        out[p++] = '0';
        return p;
    }
    uint32_t m = g.digits;
    int kept = ptext_g_strip(m);
    const int e = g.exp10;
    if (e < -4 || e >= 6) {
        for (int k = kept - 1; k >= 1; --k) {                                      // behind the point, from the last digit
            const uint32_t q = m / 10u;
            out[p + 1 + k] = (Char)('0' + (m - q * 10u));
            m = q;
        }
        out[p] = (Char)('0' + m);
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
            const uint32_t q = m / 10u;
            out[p + k + (k >= before ? 1 : 0)] = (Char)('0' + (m - q * 10u));
            m = q;
        }
        if (kept > before) out[p + before] = '.';
        return p + kept + (kept > before ? 1 : 0);
    }
    out[p++] = '0';
    out[p++] = '.';
    for (int z = -e - 1; z > 0; --z) out[p++] = '0';
    for (int k = kept - 1; k >= 0; --k) {
        const uint32_t q = m / 10u;
        out[p + k] = (Char)('0' + (m - q * 10u));
        m = q;
    }
    return p + kept;
}

// ---------------------------------------------------------------------------------------------- the lines
// tools_src/evaluate.hpp: WriteVerdict, which restates tools/SplitAlignment.cpp:596-615.

// a group that gets lines at all: the reference evaluates a default task or exits at the others
REC_HD bool ptext_has_lines(int32_t status) { return (status & (PRED_NO_TASK | PRED_OUT_OF_WINDOW)) == 0; }

// What a .seq line is made of: head "%d\t", `body` bytes of sequence (the group's own, or the tool's "N" for a group
// without a split), tail "\t0\t%lld\t%g\t%g\n".
struct ptext_seq_parts {
    ptext_g pos, min;
    int64_t count;
    int32_t head, body, tail;   // bytes
    int32_t no_split;           // the body is "N"
    int32_t ok;                 // 0: the line is the caller's (PTEXT_HOST_SEQ); the lengths are 0 then
};

// for a group with ptext_has_lines(r.status)
REC_HD ptext_seq_parts ptext_seq_parts_of(const pred_result& r)
{
    ptext_seq_parts s{};
    s.no_split = (r.status & EVAL_NO_SPLIT) != 0;
    if (!s.no_split && (r.status & EVAL_HOST_STATS)) return s;
    s.pos = ptext_g_of(s.no_split ? -1.0 : r.pos_avg);
    s.min = ptext_g_of(s.no_split ? -1.0 : r.min_avg);
    if (!s.pos.ok || !s.min.ok) return s;
    s.count = s.no_split ? 0 : r.count;
    s.head = rec_field_length(r.fusion_id);
    s.body = s.no_split ? 1 : r.seq_len;
    s.tail = 3 + rec_field_length64(s.count) + ptext_g_length(s.pos) + 1 + ptext_g_length(s.min) + 1;
    s.ok = 1;
    return s;
}

// the tail at out (room for s.tail bytes); returns its length
template <typename Char>
REC_HD int ptext_write_seq_tail(const ptext_seq_parts& s, Char* out)
{
    int p = 0;
    out[p++] = '\t';
    out[p++] = '0';
    out[p++] = '\t';
    p += rec_write_field64(s.count, out + p);
    p += ptext_g_write(s.pos, out + p);
    out[p++] = '\t';
    p += ptext_g_write(s.min, out + p);
    out[p++] = '\n';
    return p;
}

// the break position WriteBreak prints for a cluster end
REC_HD int32_t ptext_break_pos(const pred_result& r, int end) { return (r.status & EVAL_NO_SPLIT) ? 0 : r.break_pos[end]; }

// one .break line: "%d\t%d\t" name "\t+\t" / "\t-\t" "%d\n"
REC_HD int ptext_break_length(const pred_result& r, int end, int32_t name_len)
{
    return rec_field_length(r.fusion_id) + 2 + name_len + 3 + rec_field_length(ptext_break_pos(r, end));
}

template <typename Char, typename Byte>
REC_HD int ptext_write_break(const pred_result& r, int end, const Byte* name, int32_t name_len, int32_t strand, Char* out)
{
    int p = rec_write_field(r.fusion_id, out);
    p += rec_write_field(end, out + p);
    for (int32_t k = 0; k < name_len; ++k) out[p + k] = (Char)name[k];
    p += name_len;
    out[p++] = '\t';
    out[p++] = strand == 0 ? '+' : '-';
    out[p++] = '\t';
    p += rec_write_field(ptext_break_pos(r, end), out + p);
    out[p - 1] = '\n';                                                             // (rec_write_field ends a field with a tab)
    return p;
}
