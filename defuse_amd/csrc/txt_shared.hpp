// txt_shared.hpp — what text_api.hip shares with sct_api.hip: the line (and tab) tables of a text in device memory, the view of
// them a per-line kernel reads, and the integer rule of a field.  Internal: nothing here is part of the C ABI.
//
// Tables, over the text padded with zero bytes to whole 16-byte chunks:
//   (1) k_txt_count: a lane loads 16 bytes, compares them with '\n' and '\t' a dword at a time and counts by popcount; a
//       workgroup of 256 lanes (4096 bytes) leaves its two counts packed in one 64-bit word;
//   (2) a 64-bit exclusive sum over the workgroups, the totals to the host, which sizes the tables;
//   (3) k_txt_tables: the same loads and masks, a packed block scan, and every lane writes the positions of its newlines and
//       tabs at their ranks — as many as its 16 bytes hold, so a span of 2048 two-byte lines and a line that crosses many
//       spans are the same case.  Beside each newline goes the number of tabs in front of it: the tab rank its next line
//       starts with.
// With TABS false only the newlines are counted and placed, and nl_tab and tab_pos are not touched.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

namespace {

using u64 = unsigned long long;

constexpr int BLOCK = 256;
constexpr int CHUNK = 16;                     // bytes per lane
constexpr uint32_t NL4 = 0x0A0A0A0Au, TAB4 = 0x09090909u;

// 0x80 in every byte of w that equals the byte of pat, 0 elsewhere (exact: no borrow runs into a neighbour)
__device__ inline uint32_t eq_mask(uint32_t w, uint32_t pat)
{
    const uint32_t x = w ^ pat;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// ---- tables -----------------------------------------------------------------------------------------------------------

// per workgroup: newlines in the high word, tabs in the low word (4096 of either at the most)
template <bool TABS>
__global__ __launch_bounds__(BLOCK) void k_txt_count(const uint4* __restrict__ text, int64_t n_chunks, u64* __restrict__ blk)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t c = 0;
    if (i < n_chunks) {
        const uint4 v = text[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            c += (uint32_t)__popc(eq_mask(w[d], NL4)) << 16;
            if (TABS) c += (uint32_t)__popc(eq_mask(w[d], TAB4));
        }
    }
    const uint32_t sum = Reduce(tmp).Sum(c);
    if (threadIdx.x == 0) blk[blockIdx.x] = ((u64)(sum >> 16) << 32) | (u64)(sum & 0xFFFFu);
}

struct Totals {
    u64 n_nl, n_tab;
    uint32_t last;              // the last byte of the text
    uint32_t pad_;
};

__global__ void k_txt_totals(const u64* __restrict__ blk, const u64* __restrict__ blk_off, int64_t n_blocks, const uint8_t* __restrict__ text, int64_t len,
                             Totals* __restrict__ tot)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const u64 s = blk_off[n_blocks - 1] + blk[n_blocks - 1];      // (fewer than 2^31 of either: the low word does not carry)
    tot->n_nl = s >> 32;
    tot->n_tab = s & 0xFFFFFFFFull;
    tot->last = text[len - 1];
    tot->pad_ = 0;
}

template <bool TABS>
__global__ __launch_bounds__(BLOCK) void k_txt_tables(const uint4* __restrict__ text, int64_t n_chunks, const u64* __restrict__ blk_off, int64_t n_nl,
                                                      int64_t n_tab, uint32_t* __restrict__ nl_pos, uint32_t* __restrict__ nl_tab,
                                                      uint32_t* __restrict__ tab_pos)
{
    using Scan = hipcub::BlockScan<uint32_t, BLOCK>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t mn[4] = {0, 0, 0, 0}, mt[4] = {0, 0, 0, 0}, c = 0;
    if (i < n_chunks) {
        const uint4 v = text[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            mn[d] = eq_mask(w[d], NL4);
            c += (uint32_t)__popc(mn[d]) << 16;
            if (TABS) {
                mt[d] = eq_mask(w[d], TAB4);
                c += (uint32_t)__popc(mt[d]);
            }
        }
    }
    uint32_t ex;
    Scan(tmp).ExclusiveSum(c, ex);                 // (every lane of the workgroup is here)
    const u64 base = blk_off[blockIdx.x];
    int64_t kn = (int64_t)(base >> 32) + (int64_t)(ex >> 16);
    int64_t kt = (int64_t)(base & 0xFFFFFFFFull) + (int64_t)(ex & 0xFFFFu);
    const uint32_t byte0 = (uint32_t)(i * CHUNK);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        for (uint32_t m = mn[d]; m; m &= m - 1) {
            const int b = __ffs((int)m) - 1;       // bit 7, 15, 23 or 31
            if (kn < n_nl) {
                nl_pos[kn] = byte0 + 4 * d + (b >> 3);
                if (TABS) nl_tab[kn] = (uint32_t)(kt + __popc(mt[d] & ((1u << b) - 1u)));
            }
            ++kn;
        }
        if (TABS)
            for (uint32_t m = mt[d]; m; m &= m - 1) {
                if (kt < n_tab) tab_pos[kt] = byte0 + 4 * d + ((__ffs((int)m) - 1) >> 3);
                ++kt;
            }
    }
}

struct Lines {
    const uint8_t* text;
    const uint32_t* nl_pos;     // n_nl positions of '\n', ascending
    const uint32_t* nl_tab;     // tabs in front of each of them
    const uint32_t* tab_pos;    // n_tab positions of '\t', ascending
    int64_t len, n_nl, n_tab;
};

__device__ inline int64_t line_start(const Lines& L, int64_t i) { return i == 0 ? 0 : (int64_t)L.nl_pos[i - 1] + 1; }
__device__ inline int64_t line_end(const Lines& L, int64_t i) { return i < L.n_nl ? (int64_t)L.nl_pos[i] : L.len; }

// boost::lexical_cast<int> on a field: optional sign, digits only, int range (field_int of tools_src/defuse_host.hpp)
__device__ inline bool field_int(const uint8_t* __restrict__ p, int64_t n, int& out)
{
    if (n <= 0) return false;
    int64_t k = (p[0] == '+' || p[0] == '-') ? 1 : 0;
    if (k == n) return false;
    long long v = 0;
    for (; k < n; ++k) {
        if (p[k] < '0' || p[k] > '9') return false;
        v = v * 10 + (p[k] - '0');
        if (v > 2147483648LL) return false;
    }
    if (p[0] == '-') v = -v;
    if (v > 2147483647LL || v < -2147483648LL) return false;
    out = (int)v;
    return true;
}

}  // namespace
