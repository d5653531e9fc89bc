// txt_shared.hpp — what the device text readers share (text_api.hip, sct_api.hip, cmpt_api.hip, rect_api.hip, taskt_api.hip,
// taskc_api.hip): the line (and tab) tables of a text in device memory and the one host path that builds them, the view of
// them a per-line kernel reads, a line's range in the tab table, and the integer rule of a field.  Included from .hip files
// only.  Internal: nothing here is part of the C ABI.
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
// Host: text_upload_count does (1) and (2) for a text the caller has made room for, text_place_tables does (3) into tables the
// caller has made room for; what a reader does with the totals in between (a bound, a limit, growing its own arrays) is its own.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstring>
#include <string>

#include "hip_host.hpp"

namespace {

using u64 = unsigned long long;

constexpr int BLOCK = 256;
constexpr int CHUNK = 16;                     // bytes per lane
// Zeroed behind a text's last whole chunk: a reader that gathers out of its text (bat_shared.hpp) looks SRC_PAD bytes ahead
// of a line's end, and asserts TEXT_PAD >= batdev::SRC_PAD + CHUNK where it includes both headers.
constexpr size_t TEXT_PAD = 2 * CHUNK;
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

// the tabs of line i are tab_pos[first_tab_rank .. end_tab_rank), as the table beside the newlines says (unchecked)
__device__ inline int64_t first_tab_rank(const Lines& L, int64_t i) { return i == 0 ? 0 : (int64_t)L.nl_tab[i - 1]; }
__device__ inline int64_t end_tab_rank(const Lines& L, int64_t i) { return i < L.n_nl ? (int64_t)L.nl_tab[i] : L.n_tab; }

// Line i < n_lines: its bytes [s, e) and its tabs tab_pos[t0 .. t0 + n_tabs); t0 and n_tabs come from the table beside the
// newlines and are used only if they lie inside the tab table.
struct LineAt {
    int64_t s, e, t0, n_tabs;
};

__device__ inline LineAt line_at(const Lines& L, int64_t i)
{
    const int64_t t0 = first_tab_rank(L, i), t1 = end_tab_rank(L, i);
    const bool inside = t0 >= 0 && t0 <= t1 && t1 <= L.n_tab;
    return LineAt{line_start(L, i), line_end(L, i), inside ? t0 : 0, inside ? t1 - t0 : 0};
}

// what the line rules of the *_shared.hpp headers take for a line's tabs and for the integer of a field
struct TabAt {
    const uint32_t* tab_pos;    // the line's first tab
    __device__ int64_t operator()(int64_t k) const { return (int64_t)tab_pos[k]; }
};

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

struct DeviceInt {
    __device__ bool operator()(const uint8_t* p, int64_t n, int& v) const { return field_int(p, n, v); }
};

// 32-bit lengths into a 64-bit sum
struct Widen {
    __host__ __device__ u64 operator()(uint32_t v) const { return (u64)v; }
};

// ---- host: text in, tables out ------------------------------------------------------------------------------------------

// with final = 0 nothing behind the last newline is a line: a host entry does not send it up
inline int64_t whole_lines(const uint8_t* text, int64_t len)
{
    const void* nl = len ? memrchr(text, '\n', (size_t)len) : nullptr;
    return nl ? (int64_t)((const uint8_t*)nl - text) + 1 : 0;
}

inline int64_t chunks_of(int64_t len) { return (len + CHUNK - 1) / CHUNK; }
// the room a text of `len` bytes takes in device memory: whole chunks and the padding
inline size_t padded_size(int64_t len) { return (size_t)(chunks_of(len) * CHUNK) + TEXT_PAD; }

// What building a text's tables needs besides the tables; a context has one.  `tmp` is hipcub's temporary storage, which the
// context's other cub_run calls use as well.
struct TextScratch {
    hiphost::DeviceBuffer<u64, hiphost::GrowSize> blk, blk_off;
    hiphost::DeviceBuffer<Totals> totals;
    hiphost::DeviceBuffer<uint8_t, hiphost::GrowSize> tmp;
};

// `len` > 0 bytes at `src` (of `kind`) into `dst`, where the caller has padded_size(len) bytes, zeros behind them, and the
// counts of (1) and (2) into `tot`.  `start` and `up` are recorded around the upload.  The stream is synchronised once, for the
// totals.  Returns a DSA_* code, its text in `err`.
template <bool TABS>
int text_upload_count(std::string& err, TextScratch& s, uint8_t* dst, const void* src, hipMemcpyKind kind, int64_t len, hipEvent_t start, hipEvent_t up,
                      hipStream_t st, Totals& tot)
{
    const int64_t n_chunks = chunks_of(len), n_blocks = (n_chunks + BLOCK - 1) / BLOCK;
    HIPHOST_TRY(err, s.blk.reserve((size_t)n_blocks));
    HIPHOST_TRY(err, s.blk_off.reserve((size_t)n_blocks));
    HIPHOST_TRY(err, s.totals.reserve(1));
    HIPHOST_TRY(err, hipEventRecord(start, st));
    HIPHOST_TRY(err, hipMemcpyAsync(dst, src, (size_t)len, kind, st));
    HIPHOST_TRY(err, hipMemsetAsync(dst + len, 0, padded_size(len) - (size_t)len, st));
    HIPHOST_TRY(err, hipEventRecord(up, st));
    hipLaunchKernelGGL(k_txt_count<TABS>, dim3((unsigned)n_blocks), dim3(BLOCK), 0, st, reinterpret_cast<const uint4*>(dst), n_chunks, s.blk.p);
    HIPHOST_TRY(err, hiphost::cub_run(s.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, s.blk.p, s.blk_off.p, (int)n_blocks, st); }));
    hipLaunchKernelGGL(k_txt_totals, dim3(1), dim3(64), 0, st, (const u64*)s.blk.p, (const u64*)s.blk_off.p, n_blocks, (const uint8_t*)dst, len, s.totals.p);
    HIPHOST_TRY(err, hipMemcpyAsync(&tot, s.totals.p, sizeof(Totals), hipMemcpyDeviceToHost, st));
    HIPHOST_TRY(err, hipStreamSynchronize(st));
    HIPHOST_TRY(err, hipGetLastError());
    const long long n_nl = (long long)tot.n_nl, n_tab = (long long)tot.n_tab;
    if (TABS && (n_nl > len || n_tab > len)) return hiphost::fail(err, DSA_E_DEVICE, "internal: %lld newlines and %lld tabs in %lld bytes", n_nl, n_tab, (long long)len);
    if (!TABS && n_nl > len) return hiphost::fail(err, DSA_E_DEVICE, "internal: %lld newlines in %lld bytes", n_nl, (long long)len);
    return DSA_OK;
}

// (3) for the text text_upload_count left at `text`, into tables with room for tot.n_nl, tot.n_nl and tot.n_tab entries (TABS
// false: nl_pos alone, the others may be null).
template <bool TABS>
void text_place_tables(const TextScratch& s, const uint8_t* text, int64_t len, const Totals& tot, uint32_t* nl_pos, uint32_t* nl_tab, uint32_t* tab_pos,
                       hipStream_t st)
{
    const int64_t n_chunks = chunks_of(len);
    hipLaunchKernelGGL(k_txt_tables<TABS>, dim3(hiphost::grid_of(n_chunks, BLOCK)), dim3(BLOCK), 0, st, reinterpret_cast<const uint4*>(text), n_chunks,
                       (const u64*)s.blk_off.p, (int64_t)tot.n_nl, TABS ? (int64_t)tot.n_tab : (int64_t)0, nl_pos, nl_tab, tab_pos);
}

// The tables of a reader that keeps them in its context.
struct TextTables {
    hiphost::DeviceBuffer<uint32_t, hiphost::GrowSize> nl_pos, nl_tab, tab_pos;
    hipError_t reserve(const Totals& tot)
    {
        hipError_t e = nl_pos.reserve((size_t)tot.n_nl);
        if (e == hipSuccess) e = nl_tab.reserve((size_t)tot.n_nl);
        if (e == hipSuccess) e = tab_pos.reserve((size_t)tot.n_tab);
        return e;
    }
    template <bool TABS>
    Lines place(const TextScratch& s, const uint8_t* text, int64_t len, const Totals& tot, hipStream_t st) const
    {
        text_place_tables<TABS>(s, text, len, tot, nl_pos.p, nl_tab.p, tab_pos.p, st);
        return Lines{text, nl_pos.p, nl_tab.p, tab_pos.p, len, (int64_t)tot.n_nl, (int64_t)tot.n_tab};
    }
};

}  // namespace
