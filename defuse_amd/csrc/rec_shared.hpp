// rec_shared.hpp — what a split-alignment record's line is and where it sorts (include/defuse_rec.h), as __host__ __device__
// code: the kernels of rec_api.hip and a host program (tests/test_records.py) compile the same functions.
//
// The line is SplitAlignment::WriteAlignment: nine fields, each "%d" and a tab, then '\n'; pair_idx is not printed.
// The order is the pipeline's LC_ALL=C sort -n -k 1: ascending fusion id, then ascending bytes of the line.  Byte order of
// "%d\t" texts is the order of their field keys: the text read as up to 12 symbols of base 12 (tab 0, '-' 1, digits 2..11),
// left-aligned and padded with 0, because '\t' < '-' < '0'..'9' and a tab ends the shorter of two texts.  No text is a proper
// prefix of another once the tab is counted, so equal keys are equal texts.
#pragma once
#include <stdint.h>

#include "../../include/defuse_dsa.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REC_HD __host__ __device__ inline
#else
#define REC_HD inline
#endif

constexpr int REC_FIELDS = 9;                        // printed fields; dsa_record's tenth int is pair_idx
constexpr int REC_FIELD_SYMBOLS = 12;                // "-2147483648\t"
constexpr int REC_FIELD_KEY_BITS = 44;               // 12^12 < 2^44
constexpr int REC_MAX_LINE = REC_FIELDS * REC_FIELD_SYMBOLS + 1;      // 109 bytes
constexpr uint64_t REC_POW12_11 = 743008370688ull;   // 12^11: the weight of a text's first symbol
constexpr uint64_t REC_KEY_OF_0 = 2 * REC_POW12_11;  // "0\t"
constexpr uint64_t REC_KEY_OF_1 = 3 * REC_POW12_11;  // "1\t"

// unsigned order of the result is signed order of the id
REC_HD uint32_t rec_fusion_key(int32_t fusion_id) { return (uint32_t)fusion_id ^ 0x80000000u; }

// |v| without overflow at INT_MIN
REC_HD uint32_t rec_magnitude(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

// decimal digits of m, 1..10
REC_HD int rec_digits(uint32_t m)
{
    return m < 10u ? 1 : m < 100u ? 2 : m < 1000u ? 3 : m < 10000u ? 4 : m < 100000u ? 5 : m < 1000000u ? 6 : m < 10000000u ? 7
         : m < 100000000u ? 8 : m < 1000000000u ? 9 : 10;
}

// The 44-bit key of one field (file comment).  The digits come off the low end, so the text's value in base 12 is built
// upwards and then shifted left by the symbols the text does not use; the tab and the padding are zeros.
REC_HD uint64_t rec_field_key(int32_t v)
{
    uint32_t m = rec_magnitude(v);
    uint64_t text = 0, w = 1;
    int used = 1;                                    // the tab
    do {
        const uint32_t q = m / 10u;
        text += (uint64_t)(m - q * 10u + 2u) * w;
        w *= 12u;
        m = q;
        ++used;
    } while (m);
    if (v < 0) {
        text += w;                                   // '-' is symbol 1
        ++used;
    }
    text *= 12u;                                     // the tab's place
    for (; used < REC_FIELD_SYMBOLS; ++used) text *= 12u;
    return text;
}

REC_HD int rec_field_length(int32_t v) { return rec_digits(rec_magnitude(v)) + (v < 0 ? 1 : 0) + 1; }

// "%d\t" at out (or "%d" and another closing byte: the last field of a line); returns the bytes written.  Division by the
// constant 10 only (a multiplication in the ISA).
template <typename Char>
REC_HD int rec_write_field(int32_t v, Char* out, char close = '\t')
{
    uint32_t m = rec_magnitude(v);
    int p = 0;
    if (v < 0) out[p++] = '-';
    const int d = rec_digits(m);
    for (int k = d - 1; k >= 0; --k) {
        const uint32_t q = m / 10u;
        out[p + k] = (Char)('0' + (m - q * 10u));
        m = q;
    }
    out[p + d] = (Char)close;
    return p + d + 1;
}

// The same for a 64-bit value ("%lld\t"; ptext_shared.hpp prints a group's count with it): 1..19 digits.
REC_HD uint64_t rec_magnitude64(int64_t v) { return v < 0 ? 0ull - (uint64_t)v : (uint64_t)v; }

REC_HD int rec_digits64(uint64_t m)
{
    if (m < 10000000000ull) return m <= 0xFFFFFFFFull ? rec_digits((uint32_t)m) : 10;
    return 10 + rec_digits((uint32_t)(m / 10000000000ull));          // (m / 10^10 < 2^31)
}

REC_HD int rec_field_length64(int64_t v) { return rec_digits64(rec_magnitude64(v)) + (v < 0 ? 1 : 0) + 1; }

template <typename Char>
REC_HD int rec_write_field64(int64_t v, Char* out)
{
    uint64_t m = rec_magnitude64(v);
    int p = 0;
    if (v < 0) out[p++] = '-';
    const int d = rec_digits64(m);
    for (int k = d - 1; k >= 0; --k) {
        const uint64_t q = m / 10u;
        out[p + k] = (Char)('0' + (uint32_t)(m - q * 10u));
        m = q;
    }
    out[p + d] = '\t';
    return p + d + 1;
}

// the nine printed ints of a record, in print order
REC_HD const int32_t* rec_fields(const dsa_record& r) { return reinterpret_cast<const int32_t*>(&r); }

REC_HD int rec_line_length(const dsa_record& r)
{
    const int32_t* f = rec_fields(r);
    int len = 1;
    for (int k = 0; k < REC_FIELDS; ++k) len += rec_field_length(f[k]);
    return len;
}

// the line at out (room for rec_line_length(r) <= REC_MAX_LINE bytes, no terminator); returns its length
template <typename Char>
REC_HD int rec_write_line(const dsa_record& r, Char* out)
{
    const int32_t* f = rec_fields(r);
    int p = 0;
    for (int k = 0; k < REC_FIELDS; ++k) p += rec_write_field(f[k], out + p);
    out[p] = '\n';
    return p + 1;
}
