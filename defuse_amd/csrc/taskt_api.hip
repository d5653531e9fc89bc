// taskt_api.hip — the regions file and the exon table as text, parsed and resolved on gfx950 (include/defuse_task.h, section
// "region and exon text"): what a caller of task_store_create did on the host with a line splitter, lexical_cast,
// ReadAlignRegionPairs, ExonRegions::Read, ParseTranscriptID and three string maps.
//
// Both texts: the newline and tab tables of txt_shared.hpp, then one lane per line applies taskt_shared.hpp's rule.  The first
// stop is an atomic minimum over the (rare) stopping lines.
// Exon table (taskt_parse_exons):
//   lines   k_exon_lines: the rule; per line a packed count (transcripts high, exons low), the longest name
//   scan    a 64-bit exclusive sum: every transcript line's row and its first exon; totals, stop and longest name to the host
//   rows    k_exon_rows: the row of every transcript line (where its names and exon fields are), in file order
//   emit    k_exon_emit: one lane per exon; a lower bound over the rows' first exons finds its line, it reads its two fields
//   sort    the rows by transcript name and by chromosome name: stable 64-bit radix passes over big-endian 8-byte chunks of
//           the names (zero beyond their ends), last chunk first, with a pass by length in front; that is ascending byte order
//           with a prefix first.  Only as many chunks as the longest name has.  k_name_heads marks where a name differs from
//           its predecessor by comparing the bytes: a transcript that is no head is a duplicate, and stable passes leave the
//           later line there; a chromosome's head is its first line.  If a line stopped by its own rule, the rows and the
//           transcript sort are still made for the lines in front of it, and the earlier of the two stops is reported
//   number  chromosomes by first appearance (a scatter of the heads' rows, a sum over the rows), transcripts by sorted position;
//           chrom_ref and name_ref by binary search over ref_names ("gene|transcript" is read in place, the tab between the
//           two fields standing for the bar)
//   table   transcripts, exons and chrom_ref come down once and go through task_exons_create (its checks, its derived
//           columns); the sorted names stay on the device for the regions parse.
// Regions file (taskt_parse_regions):
//   lines   k_region_lines: the rule; the parsed line and its sort key (id as unsigned with the sign bit turned, then the end)
//   sort    one stable radix sort of (key, line): the lines of an (id, end) lie together in file order, the ends of an id side
//           by side, the lines without an end behind them all
//   pairs   heads of ids by a flag and an inclusive sum; k_pairs_fill writes every pair with two default ends, k_pairs_win lets
//           the last line of every (id, end) overwrite its end.  Names are resolved by binary searches: seq_names, the sorted
//           transcripts, the sorted chromosomes.
// taskt_store_create: k_pair_check finds the lowest pair task_store_create's checks refuse, then task_api.hip builds the
// store from the pairs where they are.
// Every read of a text is below its length or inside the zeroed padding of whole chunks behind it; every table is indexed
// below its count; every store is at an index below the size its buffer was reserved for.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_task.h"
#include "hip_host.hpp"
#include "taskt_shared.hpp"
#include "txt_names.hpp"
#include "txt_shared.hpp"

// task_api.hip
__attribute__((visibility("hidden"))) int taskstore_create_device(int device, const task_reference* reference, const task_exons* exons, const task_params* params,
                                                                  const task_pair* pairs_device, int64_t n, int64_t max_seq, task_store** out);

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;

thread_local std::string g_taskt_err;

#define TASKT_HIP(call) HIPHOST_TRY(g_taskt_err, call)
#define TASKT_FAIL(code, ...) hiphost::fail(g_taskt_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr u64 NO_END = 1ull << 33;            // the sort key of a line that gives no end: behind every (id, end)
constexpr int KEY_BITS = 34;

static_assert(sizeof(taskt_result) == 80 && sizeof(taskt_timing) == 40 && sizeof(taskt_region_line) == 40, "layout");
static_assert(TASKT_MAX_NAME % 8 == 0, "whole chunks");

// ---- exon table -----------------------------------------------------------------------------------------------------

struct ExonRow {                // one transcript line
    int64_t s, e;               // the line; "gene\ttranscript" is text[s, tname_off + tname_len)
    int64_t t0;                 // its first tab in the tab table
    int32_t n_tabs;
    int32_t gene_len;
    int32_t strand;
    int32_t first_exon, n_exons;
    uint32_t line;
};

struct ParseOut {
    uint32_t stop;              // in: NONE; the lowest stopping line
    uint32_t dup;               // in: NONE; the lowest line that repeats a transcript name
    uint32_t max_len;           // the longest transcript or chromosome name
    uint32_t n_valid;           // regions: lines that give an end
    u64 total;                  // exons: the packed sum over all lines
    u64 n_groups;               // exons: chromosomes; regions: pairs
    taskt_result stop_res;      // the stop's line, bytes, kind and field
};

__global__ __launch_bounds__(BLOCK) void k_exon_lines(Lines L, int64_t n_lines, u64* __restrict__ cnt, ParseOut* __restrict__ out)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t longest = 0;
    if (i < n_lines) {
        const LineAt a = line_at(L, i);
        const TabAt tab{L.tab_pos + a.t0};
        const taskt_exon_line r = taskt_parse_exon_line(L.text, a.s, a.e, a.n_tabs, tab, DeviceInt());
        cnt[i] = r.kind == 0 ? (1ull << 32) | (u64)(uint32_t)r.n_exons : 0ull;
        if (r.kind > 0) atomicMin(&out->stop, (uint32_t)i);
        if (r.kind == 0) longest = (uint32_t)max(tab(2) - tab(1), tab(1) - tab(0)) - 1u;
    }
    const uint32_t m = Reduce(tmp).Reduce(longest, hipcub::Max());      // (every lane of the workgroup is here)
    if (threadIdx.x == 0 && m) atomicMax(&out->max_len, m);
}

__global__ void k_exon_total(const u64* __restrict__ cnt, const u64* __restrict__ off, int64_t n_lines, ParseOut* __restrict__ out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) out->total = off[n_lines - 1] + cnt[n_lines - 1];
}

// The stop's line read again for its kind and field; `dup` says that it is the duplicate rule's.
template <bool EXONS>
__global__ void k_stop_result(Lines L, int64_t n_lines, uint32_t line, int dup, ParseOut* __restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || (int64_t)line >= n_lines) return;
    const LineAt a = line_at(L, line);
    const TabAt tab{L.tab_pos + a.t0};
    taskt_result r{};
    r.n_lines = line;
    r.stop_line = (int64_t)line + 1;
    r.stop_off = a.s;
    r.stop_len = a.e - a.s;
    if (EXONS) {
        const taskt_exon_line x = taskt_parse_exon_line(L.text, a.s, a.e, a.n_tabs, tab, DeviceInt());
        r.stop_kind = dup ? TASKT_EXON_DUPLICATE : x.kind;
        r.stop_field = dup ? 1 : x.field;
    } else {
        const taskt_region_line x = taskt_parse_region_line(L.text, a.s, a.e, a.n_tabs, tab, DeviceInt());
        r.stop_kind = x.kind;
        r.stop_field = x.field;
    }
    out->stop_res = r;
}

__global__ __launch_bounds__(BLOCK) void k_exon_rows(Lines L, int64_t n_lines, const u64* __restrict__ cnt, const u64* __restrict__ off, int64_t n_rows,
                                                      ExonRow* __restrict__ rows, int32_t* __restrict__ row_first, int64_t* __restrict__ tn_off,
                                                      int32_t* __restrict__ tn_len, int64_t* __restrict__ cn_off, int32_t* __restrict__ cn_len)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_lines || (cnt[i] >> 32) == 0) return;
    const int64_t r = (int64_t)(off[i] >> 32);
    if (r >= n_rows) return;
    const LineAt a = line_at(L, i);                 // a transcript line: at least five tabs
    const TabAt tab{L.tab_pos + a.t0};
    const int64_t b0 = tab(0), b1 = tab(1), b2 = tab(2);
    const taskt_exon_line x = taskt_parse_exon_line(L.text, a.s, a.e, a.n_tabs, tab, DeviceInt());
    rows[r] = ExonRow{a.s, a.e, a.t0, (int32_t)a.n_tabs, (int32_t)(b0 - a.s), x.strand, (int32_t)(uint32_t)off[i], x.n_exons, (uint32_t)i};
    row_first[r] = (int32_t)(uint32_t)off[i];
    tn_off[r] = b0 + 1;
    tn_len[r] = (int32_t)(b1 - b0 - 1);
    cn_off[r] = b1 + 1;
    cn_len[r] = (int32_t)(b2 - b1 - 1);
}

// One lane per exon: its row is the last whose first exon is not beyond it.
__global__ __launch_bounds__(BLOCK) void k_exon_emit(const uint8_t* __restrict__ text, const uint32_t* __restrict__ tab_pos, const ExonRow* __restrict__ rows,
                                                      const int32_t* __restrict__ row_first, int64_t n_rows, int64_t n_exons, task_exon* __restrict__ exons)
{
    const int64_t x = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (x >= n_exons) return;
    int64_t lo = 0, hi = n_rows;                    // the first row whose first exon is beyond x
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)row_first[mid] <= x) lo = mid + 1; else hi = mid;
    }
    task_exon ex{0, 0};
    if (lo > 0) {
        const ExonRow r = rows[lo - 1];
        const int64_t k = 4 + 2 * (x - r.first_exon);       // its fields k and k + 1; k + 1 <= n_tabs by the line's count
        if (x - r.first_exon < r.n_exons && k + 1 <= r.n_tabs) {
            const TabAt tab{tab_pos + r.t0};
            int64_t from, to;
            int v = 0;
            taskt_field(r.s, r.e, r.n_tabs, tab, k, from, to);
            (void)field_int(text + from, to - from, v);
            ex.start = v;
            taskt_field(r.s, r.e, r.n_tabs, tab, k + 1, from, to);
            (void)field_int(text + from, to - from, v);
            ex.end = v;
        }
    }
    exons[x] = ex;
}

// ---- names: sort, heads, lookups ------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void k_iota(uint32_t* __restrict__ idx, int64_t n)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n) idx[s] = (uint32_t)s;
}

// chunk < 0: the length; else the name's bytes [8 chunk, 8 chunk + 8), first byte highest, zero beyond its end
__global__ __launch_bounds__(BLOCK) void k_name_keys(const uint8_t* __restrict__ text, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                      const uint32_t* __restrict__ idx, int64_t n, int chunk, u64* __restrict__ key)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t r = idx[s];                      // (a permutation of [0, n): the sort only moves what k_iota wrote)
    const int32_t L = len[r];
    u64 k = 0;
    if (chunk < 0) k = (u64)(uint32_t)L;
    else {
        const uint8_t* __restrict__ p = text + off[r];
        for (int j = 0; j < 8; ++j) {
            const int32_t b = 8 * chunk + j;
            k = (k << 8) | (b < L ? (u64)p[b] : 0ull);
        }
    }
    key[s] = k;
}

__global__ __launch_bounds__(BLOCK) void k_name_heads(const uint8_t* __restrict__ text, const int64_t* __restrict__ off, const int32_t* __restrict__ len,
                                                       const uint32_t* __restrict__ order, int64_t n, uint32_t* __restrict__ head)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    uint32_t h = 1;
    if (s > 0) {
        const uint32_t a = order[s - 1], b = order[s];
        h = compare_bytes(text + off[a], (int64_t)len[a], text + off[b], (int64_t)len[b]) != 0 ? 1u : 0u;
    }
    head[s] = h;
}

__global__ __launch_bounds__(BLOCK) void k_tx_dups(const uint32_t* __restrict__ head, const uint32_t* __restrict__ order, const ExonRow* __restrict__ rows, int64_t n,
                                                    ParseOut* __restrict__ out)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n && !head[s]) atomicMin(&out->dup, rows[order[s]].line);
}

// the row of every chromosome's first line
__global__ __launch_bounds__(BLOCK) void k_chrom_first(const uint32_t* __restrict__ head, const uint32_t* __restrict__ order, int64_t n, uint32_t* __restrict__ first)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n && head[s]) first[order[s]] = 1u;
}

// "gene\ttranscript" read as gene + "|" + transcript
struct BarAt {
    const uint8_t* p;
    int64_t bar;
    __device__ uint8_t operator[](int64_t k) const { return k == bar ? (uint8_t)'|' : p[k]; }
};

// Sorted position s of the chromosome order: group grp[s] - 1 (grp is the inclusive sum of the heads).  A head writes its
// group's entry of the sorted list, the chromosome's number (the rank of its first row among the first rows) and chrom_ref.
__global__ __launch_bounds__(BLOCK) void k_chrom_groups(const uint8_t* __restrict__ text, const uint32_t* __restrict__ head, const uint32_t* __restrict__ grp,
                                                         const uint32_t* __restrict__ order, const uint32_t* __restrict__ rank, const int64_t* __restrict__ cn_off,
                                                         const int32_t* __restrict__ cn_len, int64_t n, NamesView ref, int64_t* __restrict__ grp_off,
                                                         int32_t* __restrict__ grp_len, int32_t* __restrict__ grp_cid, int32_t* __restrict__ chrom_ref)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n || !head[s]) return;
    const uint32_t r = order[s];
    const int64_t g = (int64_t)grp[s] - 1;                  // >= 0: position 0 is a head
    const int64_t c = rank[r];                              // below the number of groups, which is at most n
    grp_off[g] = cn_off[r];
    grp_len[g] = cn_len[r];
    grp_cid[g] = (int32_t)c;
    const int32_t found = find_name(ref, text + cn_off[r], (int64_t)cn_len[r]);
    chrom_ref[c] = found >= 0 ? found : (int32_t)(ref.n + c);
}

__global__ __launch_bounds__(BLOCK) void k_row_chrom(const uint32_t* __restrict__ grp, const uint32_t* __restrict__ order, const int32_t* __restrict__ grp_cid,
                                                      int64_t n, int32_t* __restrict__ row_chrom)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    row_chrom[order[s]] = grp_cid[grp[s] - 1];
}

// transcript s of the table is the row order[s]
__global__ __launch_bounds__(BLOCK) void k_tx_out(const uint8_t* __restrict__ text, const uint32_t* __restrict__ order, const ExonRow* __restrict__ rows,
                                                   const int32_t* __restrict__ row_chrom, const int64_t* __restrict__ tn_off, const int32_t* __restrict__ tn_len,
                                                   int64_t n, const uint32_t* __restrict__ grp, NamesView ref, task_transcript* __restrict__ tx,
                                                   int64_t* __restrict__ stn_off, int32_t* __restrict__ stn_len)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    const uint32_t r = order[s];
    const ExonRow x = rows[r];
    const int64_t n_chroms = grp[n - 1];
    const int32_t found = find_name(ref, BarAt{text + x.s, (int64_t)x.gene_len}, tn_off[r] + tn_len[r] - x.s);
    tx[s] = task_transcript{row_chrom[r], x.strand, x.first_exon, x.n_exons, found >= 0 ? found : (int32_t)(ref.n + n_chroms + s)};
    stn_off[s] = tn_off[r];
    stn_len[s] = tn_len[r];
}

// names of one text in ascending order, without repeats
struct SortedNames {
    const uint8_t* text;
    const int64_t* off;
    const int32_t* len;
    const int32_t* index;       // the number of each; NULL: its position
    int64_t n;
};

__device__ inline int32_t find_sorted(const SortedNames& S, const uint8_t* __restrict__ f, int64_t n)
{
    int64_t lo = 0, hi = S.n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (compare_bytes(S.text + S.off[mid], (int64_t)S.len[mid], f, n) < 0) lo = mid + 1; else hi = mid;
    }
    if (lo < S.n && compare_bytes(S.text + S.off[lo], (int64_t)S.len[lo], f, n) == 0) return S.index ? S.index[lo] : (int32_t)lo;
    return -1;
}

// ---- regions --------------------------------------------------------------------------------------------------------

struct Resolver {
    NamesView seqs;
    SortedNames tx, chroms;
};

// SplitAlignmentTask::Initialize's reading of a region's name (defuse_amd/task.py:pairs_from_regions)
__device__ inline task_end resolve(const Resolver& R, const uint8_t* __restrict__ name, int64_t n, int32_t strand, int32_t start, int32_t end)
{
    task_end a{-1, -1, -1, strand, start, end};
    a.seq = find_name(R.seqs, name, n);
    a.chrom = find_sorted(R.chroms, name, n);
    int64_t b0 = 0;
    while (b0 < n && name[b0] != '|') ++b0;
    if (b0 < n) {                                           // ParseTranscriptID: at least two fields; the second
        int64_t b1 = b0 + 1;
        while (b1 < n && name[b1] != '|') ++b1;
        a.transcript = find_sorted(R.tx, name + b0 + 1, b1 - b0 - 1);
    }
    return a;
}

__global__ __launch_bounds__(BLOCK) void k_region_lines(Lines L, int64_t n_lines, taskt_region_line* __restrict__ lines, u64* __restrict__ key,
                                                         uint32_t* __restrict__ idx, ParseOut* __restrict__ out)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t valid = 0;
    if (i < n_lines) {
        const LineAt a = line_at(L, i);
        const taskt_region_line r = taskt_parse_region_line(L.text, a.s, a.e, a.n_tabs, TabAt{L.tab_pos + a.t0}, DeviceInt());
        lines[i] = r;
        valid = r.kind == 0 ? 1u : 0u;
        key[i] = valid ? ((u64)((uint32_t)r.id ^ 0x80000000u) << 1) | (u64)(uint32_t)r.end : NO_END;
        idx[i] = (uint32_t)i;
        if (r.kind > 0) atomicMin(&out->stop, (uint32_t)i);
    }
    const uint32_t n = Reduce(tmp).Sum(valid);                  // (every lane of the workgroup is here)
    if (threadIdx.x == 0 && n) atomicAdd(&out->n_valid, n);
}

__global__ __launch_bounds__(BLOCK) void k_id_heads(const u64* __restrict__ skey, int64_t n_valid, uint32_t* __restrict__ head)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n_valid) head[s] = (s == 0 || (skey[s] >> 1) != (skey[s - 1] >> 1)) ? 1u : 0u;
}

// every pair with its id and two default Locations (empty name, strand 0, 0, 0)
__global__ __launch_bounds__(BLOCK) void k_pairs_fill(const u64* __restrict__ skey, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank,
                                                       int64_t n_valid, Resolver R, const uint8_t* __restrict__ text, task_pair* __restrict__ pairs,
                                                       int64_t* __restrict__ plines, ParseOut* __restrict__ out)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_valid) return;
    if (s == n_valid - 1) out->n_groups = rank[s];
    if (!head[s]) return;
    const int64_t k = (int64_t)rank[s] - 1;
    if (k < 0 || k >= n_valid) return;
    task_pair p;
    p.fusion_id = (int32_t)((uint32_t)(skey[s] >> 1) ^ 0x80000000u);
    p.end[0] = p.end[1] = resolve(R, text, 0, 0, 0, 0);
    pairs[k] = p;
    plines[2 * k] = plines[2 * k + 1] = 0;
}

// the last line of every (id, end)
__global__ __launch_bounds__(BLOCK) void k_pairs_win(const u64* __restrict__ skey, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ rank,
                                                      int64_t n_valid, int64_t n_lines, const taskt_region_line* __restrict__ lines, Resolver R,
                                                      const uint8_t* __restrict__ text, task_pair* __restrict__ pairs, int64_t* __restrict__ plines)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_valid || (s + 1 < n_valid && skey[s + 1] == skey[s])) return;
    const int64_t k = (int64_t)rank[s] - 1, i = sidx[s];
    if (k < 0 || k >= n_valid || i >= n_lines) return;
    const taskt_region_line r = lines[i];
    const int e = r.end & 1;
    pairs[k].end[e] = resolve(R, text + r.name_off, (int64_t)r.name_len, r.strand, r.start, r.stop);
    plines[2 * k + e] = i + 1;
}

__global__ __launch_bounds__(BLOCK) void k_pair_check(const task_pair* __restrict__ pairs, int64_t n, uint32_t* __restrict__ bad)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    int e;
    if (taskt_pair_fault(pairs[k], &e)) atomicMin(bad, (uint32_t)k);
}

}  // namespace

struct taskt_names : NameTable {};

struct taskt_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[8];       // 0-2 exons: start, text up, kernels done; 3-5 regions likewise; 6, 7 around the pairs' checks
    taskt_timing timing{};
    // the text tables and the scratch of either parse
    TextScratch scratch;
    TextTables tables;
    DeviceBuffer<ParseOut> out;
    DeviceBuffer<u64, GrowSize> cnt, cnt_off, key[2];
    DeviceBuffer<uint32_t, GrowSize> idx[2], head, grp, first, rank;
    Lines L{};
    int64_t n_lines = 0;
    // where device-to-host copies on the stream land: they outlive every frame that queues them
    Totals h_tot{};
    ParseOut h_out{};
    u64 h_before = 0;
    uint32_t h_groups = 0;
    std::vector<int32_t> h_stn_len;
    DeviceBuffer<uint32_t, GrowSize> tx_order;
    // the exon table: its text stays (the names are read in place), the sorted lists for the regions' lookups
    DeviceBuffer<uint8_t, GrowSize> etext;
    DeviceBuffer<ExonRow, GrowSize> rows;
    DeviceBuffer<int32_t, GrowSize> row_first, tn_len, cn_len, row_chrom, grp_len, grp_cid, stn_len, chrom_ref;
    DeviceBuffer<int64_t, GrowSize> tn_off, cn_off, grp_off, stn_off;
    DeviceBuffer<task_transcript, GrowSize> tx;
    DeviceBuffer<task_exon, GrowSize> dexons;
    task_exons* exons = nullptr;
    int64_t etext_len = 0, n_tx = 0, n_chroms = 0, name_bytes = 0;
    std::vector<task_transcript> h_tx;
    std::vector<task_exon> h_exons;
    std::vector<int32_t> h_chrom_ref;
    // the regions
    DeviceBuffer<uint8_t, GrowSize> rtext;
    DeviceBuffer<taskt_region_line, GrowSize> lines;
    DeviceBuffer<task_pair, GrowSize> pairs;
    DeviceBuffer<int64_t, GrowSize> plines;
    bool has_pairs = false;
    int64_t n_pairs = 0, n_seq_names = 0;
};

namespace {

void drop_exons(taskt_ctx* c)
{
    if (c->exons) task_exons_destroy(c->exons);
    c->exons = nullptr;
    c->n_tx = c->n_chroms = c->name_bytes = c->etext_len = 0;
    c->h_tx.clear();
    c->h_exons.clear();
    c->h_chrom_ref.clear();
    c->has_pairs = false;
    c->n_pairs = 0;
}

// The text (len > 0) into `text` with its padding, and its line and tab tables; leaves c->L and c->n_lines.  `kind` says
// where `host` points: host memory, or memory of the ctx's device whose writer has finished.
int load_text(taskt_ctx* c, DeviceBuffer<uint8_t, GrowSize>& text, const uint8_t* host, int64_t len, hipEvent_t start, hipEvent_t up,
              hipMemcpyKind kind = hipMemcpyHostToDevice)
{
    hipStream_t st = c->st;
    TASKT_HIP(text.reserve(padded_size(len)));
    TASKT_HIP(c->out.reserve(1));
    Totals& tot = c->h_tot;
    if (const int rc = text_upload_count<true>(g_taskt_err, c->scratch, text.p, host, kind, len, start, up, st, tot)) return rc;
    TASKT_HIP(c->tables.reserve(tot));
    c->L = c->tables.place<true>(c->scratch, text.p, len, tot, st);
    c->n_lines = (int64_t)tot.n_nl + (tot.last != '\n' ? 1 : 0);         // at least one: the text is not empty
    c->h_out = ParseOut{};
    c->h_out.stop = c->h_out.dup = NONE;
    TASKT_HIP(hipMemcpyAsync(c->out.p, &c->h_out, sizeof(ParseOut), hipMemcpyHostToDevice, st));
    return DSA_OK;
}

// The result of a stop at `line`, from the device.
template <bool EXONS>
int stop_result(taskt_ctx* c, uint32_t line, int dup, taskt_result* result)
{
    hipStream_t st = c->st;
    hipLaunchKernelGGL(k_stop_result<EXONS>, dim3(1), dim3(64), 0, st, c->L, c->n_lines, line, dup, c->out.p);
    ParseOut& out = c->h_out;
    TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
    TASKT_HIP(hipStreamSynchronize(st));
    TASKT_HIP(hipGetLastError());
    const taskt_result& r = out.stop_res;
    if (r.stop_line != (int64_t)line + 1 || r.stop_kind <= 0 || r.stop_off < 0 || r.stop_len < 0 || r.stop_off + r.stop_len > c->L.len)
        return TASKT_FAIL(DSA_E_DEVICE, "internal: a stop at line %u that is none", line + 1);
    *result = r;
    return DSA_OK;
}

// order[s] = the item at sorted position s of n names (off, len) of `text`, none longer than max_len <= TASKT_MAX_NAME:
// ascending bytes, a prefix first, equal names in item order.  Returns the buffer (one of c->idx) in *order.
int sort_names(taskt_ctx* c, const uint8_t* text, const int64_t* off, const int32_t* len, int64_t n, int max_len, const uint32_t** order)
{
    hipStream_t st = c->st;
    for (int k = 0; k < 2; ++k) {
        TASKT_HIP(c->key[k].reserve((size_t)n));
        TASKT_HIP(c->idx[k].reserve((size_t)n));
    }
    int cur = 0;
    hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(BLOCK), 0, st, c->idx[0].p, n);
    const int chunks = (max_len + 7) / 8;
    for (int pass = -1; pass < chunks; ++pass) {
        const int chunk = pass < 0 ? -1 : chunks - 1 - pass;
        hipLaunchKernelGGL(k_name_keys, dim3(grid_of(n)), dim3(BLOCK), 0, st, text, off, len, (const uint32_t*)c->idx[cur].p, n, chunk, c->key[0].p);
        TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->key[0].p, c->key[1].p, (const uint32_t*)c->idx[cur].p, c->idx[1 - cur].p, (int)n, 0,
                                                      chunk < 0 ? 8 : 64, st);
        }));
        cur = 1 - cur;
    }
    *order = c->idx[cur].p;
    return DSA_OK;
}

int parse_exons(taskt_ctx* c, const taskt_names* ref, const uint8_t* text, int64_t len, taskt_result* result)
{
    hipStream_t st = c->st;
    if (const int rc = load_text(c, c->etext, text, len, c->ev[0], c->ev[1])) return rc;
    const Lines L = c->L;
    const int64_t n_lines = c->n_lines;
    TASKT_HIP(c->cnt.reserve((size_t)n_lines));
    TASKT_HIP(c->cnt_off.reserve((size_t)n_lines));
    hipLaunchKernelGGL(k_exon_lines, dim3(grid_of(n_lines)), dim3(BLOCK), 0, st, L, n_lines, c->cnt.p, c->out.p);
    TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->cnt.p, c->cnt_off.p, (int)n_lines, st); }));
    hipLaunchKernelGGL(k_exon_total, dim3(1), dim3(64), 0, st, (const u64*)c->cnt.p, (const u64*)c->cnt_off.p, n_lines, c->out.p);
    ParseOut& out = c->h_out;
    TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
    TASKT_HIP(hipStreamSynchronize(st));
    TASKT_HIP(hipGetLastError());
    // With a stop by a line's own rule the duplicate rule is still owed to the transcript lines in front of it: `used` lines
    // are looked at, and their counts are the exclusive sum at the stop.
    const bool stopped = (int64_t)out.stop < n_lines;
    const uint32_t stop = out.stop;
    const int64_t used = stopped ? (int64_t)stop : n_lines;
    c->h_before = out.total;
    if (stopped) {
        TASKT_HIP(hipMemcpyAsync(&c->h_before, c->cnt_off.p + stop, sizeof(u64), hipMemcpyDeviceToHost, st));
        TASKT_HIP(hipStreamSynchronize(st));
    }
    const int64_t n_rows = (int64_t)(c->h_before >> 32), n_exons = (int64_t)(c->h_before & 0xFFFFFFFFull);
    const int max_len = (int)out.max_len;
    if (n_rows > used || n_exons > len || max_len > TASKT_MAX_NAME)
        return TASKT_FAIL(DSA_E_DEVICE, "internal: %lld transcripts and %lld exons in %lld lines", (long long)n_rows, (long long)n_exons, (long long)used);
    int64_t n_chroms = 0;
    c->h_tx.assign((size_t)n_rows, task_transcript{});
    c->h_exons.assign((size_t)n_exons, task_exon{});
    c->h_stn_len.assign((size_t)n_rows, 0);
    if (n_rows) {
        TASKT_HIP(c->rows.reserve((size_t)n_rows));
        for (auto* b : {&c->row_first, &c->tn_len, &c->cn_len, &c->row_chrom, &c->grp_len, &c->grp_cid, &c->stn_len, &c->chrom_ref}) TASKT_HIP(b->reserve((size_t)n_rows));
        for (auto* b : {&c->tn_off, &c->cn_off, &c->grp_off, &c->stn_off}) TASKT_HIP(b->reserve((size_t)n_rows));
        for (auto* b : {&c->head, &c->grp, &c->first, &c->rank, &c->tx_order}) TASKT_HIP(b->reserve((size_t)n_rows));
        TASKT_HIP(c->tx.reserve((size_t)n_rows));
        TASKT_HIP(c->dexons.reserve((size_t)n_exons));
        hipLaunchKernelGGL(k_exon_rows, dim3(grid_of(used)), dim3(BLOCK), 0, st, L, used, (const u64*)c->cnt.p, (const u64*)c->cnt_off.p, n_rows, c->rows.p,
                           c->row_first.p, c->tn_off.p, c->tn_len.p, c->cn_off.p, c->cn_len.p);
        // transcripts: their sorted position is their number; a name that is no head repeats an earlier line's
        const uint32_t* order = nullptr;
        if (const int rc = sort_names(c, L.text, c->tn_off.p, c->tn_len.p, n_rows, max_len, &order)) return rc;
        hipLaunchKernelGGL(k_name_heads, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, L.text, (const int64_t*)c->tn_off.p, (const int32_t*)c->tn_len.p, order, n_rows,
                           c->head.p);
        hipLaunchKernelGGL(k_tx_dups, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, (const uint32_t*)c->head.p, order, (const ExonRow*)c->rows.p, n_rows, c->out.p);
        TASKT_HIP(hipMemcpyAsync(c->tx_order.p, order, (size_t)n_rows * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));      // (the next sort takes the buffers)
    }
    if (stopped) {                                  // the earlier of the two stops; nothing else of the table is made
        if (n_rows) {
            TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
            TASKT_HIP(hipStreamSynchronize(st));
            TASKT_HIP(hipGetLastError());
            if (out.dup < stop) return stop_result<true>(c, out.dup, 1, result);
        }
        return stop_result<true>(c, stop, 0, result);
    }
    result->n_lines = n_lines;
    result->n_skipped = n_lines - n_rows;
    if (n_rows) {
        hipLaunchKernelGGL(k_exon_emit, dim3(grid_of(n_exons)), dim3(BLOCK), 0, st, L.text, L.tab_pos, (const ExonRow*)c->rows.p, (const int32_t*)c->row_first.p,
                           n_rows, n_exons, c->dexons.p);
        // chromosomes: groups of equal names, numbered by their first rows
        const uint32_t* order = nullptr;
        if (const int rc = sort_names(c, L.text, c->cn_off.p, c->cn_len.p, n_rows, max_len, &order)) return rc;
        hipLaunchKernelGGL(k_name_heads, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, L.text, (const int64_t*)c->cn_off.p, (const int32_t*)c->cn_len.p, order, n_rows,
                           c->head.p);
        TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->head.p, c->grp.p, (int)n_rows, st); }));
        TASKT_HIP(hipMemsetAsync(c->first.p, 0, (size_t)n_rows * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_chrom_first, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, (const uint32_t*)c->head.p, order, n_rows, c->first.p);
        TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->first.p, c->rank.p, (int)n_rows, st); }));
        hipLaunchKernelGGL(k_chrom_groups, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, L.text, (const uint32_t*)c->head.p, (const uint32_t*)c->grp.p, order,
                           (const uint32_t*)c->rank.p, (const int64_t*)c->cn_off.p, (const int32_t*)c->cn_len.p, n_rows, ref->view(), c->grp_off.p, c->grp_len.p,
                           c->grp_cid.p, c->chrom_ref.p);
        hipLaunchKernelGGL(k_row_chrom, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, (const uint32_t*)c->grp.p, order, (const int32_t*)c->grp_cid.p, n_rows,
                           c->row_chrom.p);
        TASKT_HIP(hipMemcpyAsync(&c->h_groups, c->grp.p + (n_rows - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        hipLaunchKernelGGL(k_tx_out, dim3(grid_of(n_rows)), dim3(BLOCK), 0, st, L.text, (const uint32_t*)c->tx_order.p, (const ExonRow*)c->rows.p,
                           (const int32_t*)c->row_chrom.p, (const int64_t*)c->tn_off.p, (const int32_t*)c->tn_len.p, n_rows, (const uint32_t*)c->grp.p, ref->view(), c->tx.p,
                           c->stn_off.p, c->stn_len.p);
        TASKT_HIP(hipEventRecord(c->ev[2], st));
        TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
        TASKT_HIP(hipStreamSynchronize(st));
        TASKT_HIP(hipGetLastError());
        if ((int64_t)out.dup < n_lines) return stop_result<true>(c, out.dup, 1, result);
        n_chroms = c->h_groups;
        if (n_chroms < 1 || n_chroms > n_rows) return TASKT_FAIL(DSA_E_DEVICE, "internal: %lld chromosomes of %lld transcripts", (long long)n_chroms, (long long)n_rows);
        if (ref->n + n_chroms + n_rows > (int64_t)INT32_MAX)
            return TASKT_FAIL(DSA_E_LIMIT, "%lld names, %lld chromosomes and %lld transcripts: more than 2^31 - 1 reference numbers", (long long)ref->n,
                              (long long)n_chroms, (long long)n_rows);
        TASKT_HIP(hipMemcpyAsync(c->h_tx.data(), c->tx.p, (size_t)n_rows * sizeof(task_transcript), hipMemcpyDeviceToHost, st));
        if (n_exons) TASKT_HIP(hipMemcpyAsync(c->h_exons.data(), c->dexons.p, (size_t)n_exons * sizeof(task_exon), hipMemcpyDeviceToHost, st));
        TASKT_HIP(hipMemcpyAsync(c->h_stn_len.data(), c->stn_len.p, (size_t)n_rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        TASKT_HIP(hipEventRecord(c->ev[2], st));
    }
    c->h_chrom_ref.assign((size_t)n_chroms, 0);
    if (n_chroms) TASKT_HIP(hipMemcpyAsync(c->h_chrom_ref.data(), c->chrom_ref.p, (size_t)n_chroms * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TASKT_HIP(hipStreamSynchronize(st));
    if (const int rc = task_exons_create(c->device, c->h_chrom_ref.data(), (int32_t)n_chroms, c->h_tx.data(), (int32_t)n_rows, c->h_exons.data(), n_exons, &c->exons))
        return TASKT_FAIL(rc, "taskt_parse_exons: %s", task_last_error());
    TASKT_HIP(hipSetDevice(c->device));
    c->etext_len = len;
    c->n_tx = n_rows;
    c->n_chroms = n_chroms;
    c->name_bytes = 0;
    for (const int32_t l : c->h_stn_len) c->name_bytes += l;
    result->n_items = n_rows;
    result->n_exons = n_exons;
    result->n_chroms = n_chroms;
    result->name_bytes = c->name_bytes;
    return DSA_OK;
}

Resolver resolver(const taskt_ctx* c, const taskt_names* seqs)
{
    return Resolver{seqs->view(), SortedNames{c->etext.p, c->stn_off.p, c->stn_len.p, nullptr, c->n_tx},
                    SortedNames{c->etext.p, c->grp_off.p, c->grp_len.p, c->grp_cid.p, c->n_chroms}};
}

int parse_regions(taskt_ctx* c, const taskt_names* seqs, const uint8_t* text, int64_t len, hipMemcpyKind kind, taskt_result* result)
{
    hipStream_t st = c->st;
    if (const int rc = load_text(c, c->rtext, text, len, c->ev[3], c->ev[4], kind)) return rc;
    const Lines L = c->L;
    const int64_t n_lines = c->n_lines;
    TASKT_HIP(c->lines.reserve((size_t)n_lines));
    for (int k = 0; k < 2; ++k) {
        TASKT_HIP(c->key[k].reserve((size_t)n_lines));
        TASKT_HIP(c->idx[k].reserve((size_t)n_lines));
    }
    hipLaunchKernelGGL(k_region_lines, dim3(grid_of(n_lines)), dim3(BLOCK), 0, st, L, n_lines, c->lines.p, c->key[0].p, c->idx[0].p, c->out.p);
    ParseOut& out = c->h_out;
    TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
    TASKT_HIP(hipStreamSynchronize(st));
    TASKT_HIP(hipGetLastError());
    if ((int64_t)out.stop < n_lines) return stop_result<false>(c, out.stop, 0, result);
    const int64_t n_valid = out.n_valid;
    if (n_valid > n_lines) return TASKT_FAIL(DSA_E_DEVICE, "internal: %lld ends in %lld lines", (long long)n_valid, (long long)n_lines);
    int64_t n_pairs = 0;
    if (n_valid) {
        TASKT_HIP(c->head.reserve((size_t)n_valid));
        TASKT_HIP(c->rank.reserve((size_t)n_valid));
        TASKT_HIP(c->pairs.reserve((size_t)n_valid));
        TASKT_HIP(c->plines.reserve(2 * (size_t)n_valid));
        TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->key[0].p, c->key[1].p, (const uint32_t*)c->idx[0].p, c->idx[1].p, (int)n_lines, 0, KEY_BITS,
                                                      st);
        }));
        const Resolver R = resolver(c, seqs);
        hipLaunchKernelGGL(k_id_heads, dim3(grid_of(n_valid)), dim3(BLOCK), 0, st, (const u64*)c->key[1].p, n_valid, c->head.p);
        TASKT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->head.p, c->rank.p, (int)n_valid, st); }));
        hipLaunchKernelGGL(k_pairs_fill, dim3(grid_of(n_valid)), dim3(BLOCK), 0, st, (const u64*)c->key[1].p, (const uint32_t*)c->head.p, (const uint32_t*)c->rank.p,
                           n_valid, R, L.text, c->pairs.p, c->plines.p, c->out.p);
        hipLaunchKernelGGL(k_pairs_win, dim3(grid_of(n_valid)), dim3(BLOCK), 0, st, (const u64*)c->key[1].p, (const uint32_t*)c->idx[1].p, (const uint32_t*)c->rank.p,
                           n_valid, n_lines, (const taskt_region_line*)c->lines.p, R, L.text, c->pairs.p, c->plines.p);
        TASKT_HIP(hipEventRecord(c->ev[5], st));
        TASKT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(ParseOut), hipMemcpyDeviceToHost, st));
        TASKT_HIP(hipStreamSynchronize(st));
        TASKT_HIP(hipGetLastError());
        n_pairs = (int64_t)out.n_groups;
        if (n_pairs < 1 || n_pairs > n_valid) return TASKT_FAIL(DSA_E_DEVICE, "internal: %lld pairs of %lld ends", (long long)n_pairs, (long long)n_valid);
    } else {
        TASKT_HIP(c->pairs.reserve(1));
        TASKT_HIP(c->plines.reserve(2));
        TASKT_HIP(hipEventRecord(c->ev[5], st));
        TASKT_HIP(hipStreamSynchronize(st));
    }
    c->has_pairs = true;
    c->n_pairs = n_pairs;
    c->n_seq_names = seqs->n;
    result->n_lines = n_lines;
    result->n_skipped = n_lines - n_valid;
    result->n_items = n_pairs;
    return DSA_OK;
}

// what both parse calls check before a device is touched; leaves the empty result
int check_text(const char* fn, const void* ctx, const void* names, const uint8_t* text, int64_t len, taskt_result* result)
{
    if (!result) return TASKT_FAIL(DSA_E_ARG, "%s: no result", fn);
    *result = taskt_result{};
    result->stop_field = -1;
    if (len < 0) return TASKT_FAIL(DSA_E_ARG, "%s: negative length (%lld)", fn, (long long)len);
    if (len > (int64_t)INT32_MAX) return TASKT_FAIL(DSA_E_LIMIT, "%s: a text of %lld bytes, more than 2^31 - 1", fn, (long long)len);
    if (len && !text) return TASKT_FAIL(DSA_E_ARG, "%s: null pointer with non-zero size", fn);
    if (!ctx || !names) return TASKT_FAIL(DSA_E_ARG, "%s: no %s", fn, !ctx ? "ctx" : "names");
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* taskt_last_error(void) { return g_taskt_err.c_str(); }

int taskt_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names, taskt_names** out)
{
    if (!out) return TASKT_FAIL(DSA_E_ARG, "taskt_names_create: no output");
    *out = nullptr;
    taskt_names* nm = new taskt_names();
    if (const int rc = name_table_create(g_taskt_err, "taskt_names_create", device, name_bytes, name_bytes_len, name_off, n_names, nm)) {
        delete nm;
        return rc;
    }
    *out = nm;
    return DSA_OK;
}

void taskt_names_destroy(taskt_names* names)
{
    if (!names) return;
    (void)hipSetDevice(names->device);
    delete names;
}

int taskt_create(int device, taskt_ctx** out)
{
    if (!out) return TASKT_FAIL(DSA_E_ARG, "taskt_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_taskt_err)) return DSA_E_DEVICE;
    TASKT_HIP(hipSetDevice(device));
    taskt_ctx* c = new taskt_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return TASKT_FAIL(DSA_E_DEVICE, "taskt_create: cannot create a stream or an event");
    }
    *out = c;
    return DSA_OK;
}

void taskt_destroy(taskt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    drop_exons(c);
    (void)hipSetDevice(c->device);
    delete c;
}

int taskt_parse_exons(taskt_ctx* c, const taskt_names* ref_names, const uint8_t* text, int64_t len, taskt_result* result)
{
    if (const int rc = check_text("taskt_parse_exons", c, ref_names, text, len, result)) return rc;
    if (c->device != ref_names->device) return TASKT_FAIL(DSA_E_ARG, "taskt_parse_exons: ctx and names are on devices %d and %d", c->device, ref_names->device);
    TASKT_HIP(hipSetDevice(c->device));
    drop_exons(c);
    TASKT_HIP(hipSetDevice(c->device));
    c->timing.exon_upload_ms = c->timing.exon_device_ms = c->timing.exon_table_ms = 0.f;
    c->timing.exon_bytes = len;
    int rc;
    if (len == 0) {                                 // no line: the empty table
        rc = task_exons_create(c->device, nullptr, 0, nullptr, 0, nullptr, 0, &c->exons);
        if (rc) return TASKT_FAIL(rc, "taskt_parse_exons: %s", task_last_error());
        return DSA_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    rc = parse_exons(c, ref_names, text, len, result);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);          // nothing of a refused call is in flight when it returns
        drop_exons(c);
        return rc;
    }
    const float wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->timing.exon_upload_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.exon_device_ms = result->stop_line ? 0.f : hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.exon_table_ms = result->stop_line ? 0.f : std::max(0.f, wall - c->timing.exon_upload_ms - c->timing.exon_device_ms);
    return DSA_OK;
}

}  // extern "C"

// taskt_parse_regions, and for taskc_api.hip the same over a text that lies in the memory of the ctx's device and whose writer
// has finished (no public header has this one; the message is taskt_last_error's).
static int parse_regions_from(taskt_ctx* c, const taskt_names* seq_names, const uint8_t* text, int64_t len, hipMemcpyKind kind, taskt_result* result)
{
    if (const int rc = check_text("taskt_parse_regions", c, seq_names, text, len, result)) return rc;
    if (c->device != seq_names->device) return TASKT_FAIL(DSA_E_ARG, "taskt_parse_regions: ctx and names are on devices %d and %d", c->device, seq_names->device);
    if (!c->exons) return TASKT_FAIL(DSA_E_ARG, "taskt_parse_regions: the ctx has no exon table (taskt_parse_exons first)");
    TASKT_HIP(hipSetDevice(c->device));
    c->has_pairs = false;
    c->n_pairs = 0;
    c->timing.region_upload_ms = c->timing.region_device_ms = c->timing.check_ms = 0.f;
    c->timing.region_bytes = len;
    if (len == 0) {                                 // no line: no pair
        TASKT_HIP(c->pairs.reserve(1));
        TASKT_HIP(c->plines.reserve(2));
        c->has_pairs = true;
        c->n_seq_names = seq_names->n;
        return DSA_OK;
    }
    const int rc = parse_regions(c, seq_names, text, len, kind, result);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->has_pairs = false;
        return rc;
    }
    c->timing.region_upload_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    c->timing.region_device_ms = result->stop_line ? 0.f : hiphost::elapsed(c->ev[4], c->ev[5]);
    return DSA_OK;
}

__attribute__((visibility("hidden"))) int taskt_regions_from_device(taskt_ctx* c, const taskt_names* seq_names, int device, const uint8_t* text, int64_t len,
                                                                    taskt_result* result)
{
    if (c && c->device != device) return TASKT_FAIL(DSA_E_ARG, "taskt_parse_regions: the text is on device %d, the ctx on %d", device, c->device);
    return parse_regions_from(c, seq_names, text, len, hipMemcpyDeviceToDevice, result);
}

extern "C" {

int taskt_parse_regions(taskt_ctx* c, const taskt_names* seq_names, const uint8_t* text, int64_t len, taskt_result* result)
{
    return parse_regions_from(c, seq_names, text, len, hipMemcpyHostToDevice, result);
}

const task_exons* taskt_exons(const taskt_ctx* c) { return c ? c->exons : nullptr; }

int taskt_exons_fetch(taskt_ctx* c, task_transcript* transcripts, int64_t transcripts_cap, task_exon* exons, int64_t exons_cap, int32_t* chrom_ref, int64_t chrom_cap,
                      int64_t* name_off, int64_t name_off_cap, uint8_t* name_bytes, int64_t name_bytes_cap)
{
    if (transcripts_cap < 0 || exons_cap < 0 || chrom_cap < 0 || name_off_cap < 0 || name_bytes_cap < 0) return TASKT_FAIL(DSA_E_ARG, "taskt_exons_fetch: negative capacity");
    if ((transcripts_cap && !transcripts) || (exons_cap && !exons) || (chrom_cap && !chrom_ref) || (name_off_cap && !name_off) || (name_bytes_cap && !name_bytes))
        return TASKT_FAIL(DSA_E_ARG, "taskt_exons_fetch: capacity without a buffer");
    if (!c) return TASKT_FAIL(DSA_E_ARG, "taskt_exons_fetch: no ctx");
    if (!c->exons) return TASKT_FAIL(DSA_E_ARG, "taskt_exons_fetch: the ctx has no exon table");
    const int64_t n_exons = (int64_t)c->h_exons.size();
    if ((transcripts && transcripts_cap < c->n_tx) || (exons && exons_cap < n_exons) || (chrom_ref && chrom_cap < c->n_chroms) ||
        (name_off && name_off_cap < c->n_tx + 1) || (name_bytes && name_bytes_cap < c->name_bytes))
        return TASKT_FAIL(DSA_E_CAPACITY, "the table has %lld transcripts, %lld exons, %lld chromosomes and %lld name bytes", (long long)c->n_tx, (long long)n_exons,
                          (long long)c->n_chroms, (long long)c->name_bytes);
    std::vector<int64_t> off((size_t)c->n_tx);
    std::vector<int32_t> len((size_t)c->n_tx);
    std::vector<uint8_t> text((size_t)c->etext_len);
    if ((name_off || name_bytes) && c->n_tx) {
        TASKT_HIP(hipSetDevice(c->device));
        TASKT_HIP(hipMemcpyAsync(off.data(), c->stn_off.p, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
        TASKT_HIP(hipMemcpyAsync(len.data(), c->stn_len.p, len.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
        TASKT_HIP(hipMemcpyAsync(text.data(), c->etext.p, text.size(), hipMemcpyDeviceToHost, c->st));
        TASKT_HIP(hipStreamSynchronize(c->st));
        int64_t at = 0;
        for (int64_t t = 0; t < c->n_tx; ++t) {
            if (off[(size_t)t] < 0 || len[(size_t)t] < 0 || off[(size_t)t] + len[(size_t)t] > c->etext_len || at + len[(size_t)t] > c->name_bytes)
                return TASKT_FAIL(DSA_E_DEVICE, "internal: the name of transcript %lld lies outside the text", (long long)t);
            at += len[(size_t)t];
        }
    }
    if (transcripts && c->n_tx) memcpy(transcripts, c->h_tx.data(), (size_t)c->n_tx * sizeof(task_transcript));
    if (exons && n_exons) memcpy(exons, c->h_exons.data(), (size_t)n_exons * sizeof(task_exon));
    if (chrom_ref && c->n_chroms) memcpy(chrom_ref, c->h_chrom_ref.data(), (size_t)c->n_chroms * sizeof(int32_t));
    int64_t at = 0;
    for (int64_t t = 0; t < c->n_tx; ++t) {
        if (name_off) name_off[t] = at;
        if (name_bytes && len[(size_t)t]) memcpy(name_bytes + at, text.data() + off[(size_t)t], (size_t)len[(size_t)t]);
        at += len[(size_t)t];
    }
    if (name_off) name_off[c->n_tx] = at;
    return DSA_OK;
}

int taskt_pairs_fetch(taskt_ctx* c, task_pair* pairs, int64_t pairs_cap, int64_t* lines, int64_t lines_cap)
{
    if (pairs_cap < 0 || lines_cap < 0) return TASKT_FAIL(DSA_E_ARG, "taskt_pairs_fetch: negative capacity");
    if ((pairs_cap && !pairs) || (lines_cap && !lines)) return TASKT_FAIL(DSA_E_ARG, "taskt_pairs_fetch: capacity without a buffer");
    if (!c) return TASKT_FAIL(DSA_E_ARG, "taskt_pairs_fetch: no ctx");
    if (!c->has_pairs) return TASKT_FAIL(DSA_E_ARG, "taskt_pairs_fetch: the ctx has no pairs");
    if ((pairs && pairs_cap < c->n_pairs) || (lines && lines_cap < 2 * c->n_pairs)) return TASKT_FAIL(DSA_E_CAPACITY, "the ctx has %lld pairs", (long long)c->n_pairs);
    if (c->n_pairs == 0) return DSA_OK;
    TASKT_HIP(hipSetDevice(c->device));
    if (pairs) TASKT_HIP(hipMemcpyAsync(pairs, c->pairs.p, (size_t)c->n_pairs * sizeof(task_pair), hipMemcpyDeviceToHost, c->st));
    if (lines) TASKT_HIP(hipMemcpyAsync(lines, c->plines.p, 2 * (size_t)c->n_pairs * sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
    TASKT_HIP(hipStreamSynchronize(c->st));
    return DSA_OK;
}

int taskt_store_create(taskt_ctx* c, const task_reference* reference, const task_params* params, task_store** out)
{
    if (!out) return TASKT_FAIL(DSA_E_ARG, "taskt_store_create: no output");
    *out = nullptr;
    if (!c || !reference || !params) return TASKT_FAIL(DSA_E_ARG, "taskt_store_create: no %s", !c ? "ctx" : !reference ? "reference" : "params");
    if (!c->exons || !c->has_pairs) return TASKT_FAIL(DSA_E_ARG, "taskt_store_create: the ctx has no %s", !c->exons ? "exon table" : "pairs");
    if (c->n_pairs > (int64_t)INT32_MAX / 2) return TASKT_FAIL(DSA_E_LIMIT, "more than 2^30 - 1 pairs in one store");
    TASKT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    c->timing.check_ms = 0.f;
    if (c->n_pairs) {
        const uint32_t none = NONE;
        uint32_t bad = NONE;
        uint32_t* flag = &c->out.p->stop;
        TASKT_HIP(hipEventRecord(c->ev[6], st));
        TASKT_HIP(hipMemcpyAsync(flag, &none, sizeof none, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pair_check, dim3(grid_of(c->n_pairs)), dim3(BLOCK), 0, st, (const task_pair*)c->pairs.p, c->n_pairs, flag);
        TASKT_HIP(hipEventRecord(c->ev[7], st));
        TASKT_HIP(hipMemcpyAsync(&bad, flag, sizeof bad, hipMemcpyDeviceToHost, st));
        TASKT_HIP(hipStreamSynchronize(st));
        TASKT_HIP(hipGetLastError());
        c->timing.check_ms = hiphost::elapsed(c->ev[6], c->ev[7]);
        if ((int64_t)bad < c->n_pairs) {
            task_pair p{};
            int64_t lines[2] = {0, 0};
            TASKT_HIP(hipMemcpy(&p, c->pairs.p + bad, sizeof p, hipMemcpyDeviceToHost));
            TASKT_HIP(hipMemcpy(lines, c->plines.p + 2 * (size_t)bad, sizeof lines, hipMemcpyDeviceToHost));
            int e = 0;
            const int fault = taskt_pair_fault(p, &e);
            const task_end& a = p.end[e];
            if (fault == 1)
                return TASKT_FAIL(DSA_E_ARG, "pair %u (lines %lld and %lld): fusion_id %d is outside [0, 2^31)", bad, (long long)lines[0], (long long)lines[1], p.fusion_id);
            if (fault == 2)
                return TASKT_FAIL(DSA_E_LIMIT, "pair %u (fusion_id %d, line %lld): end[%d] (%d, %d) has a coordinate beyond +-%d", bad, p.fusion_id, (long long)lines[e], e,
                                  a.start, a.end, TASK_MAX_COORD);
            if (fault == 3)
                return TASKT_FAIL(DSA_E_LIMIT, "pair %u (fusion_id %d, line %lld): end[%d] (%d, %d) spans more than %d bases", bad, p.fusion_id, (long long)lines[e], e, a.start,
                                  a.end, TASK_MAX_REGION);
            return TASKT_FAIL(DSA_E_DEVICE, "internal: pair %u was refused without a cause", bad);
        }
    }
    const int rc = taskstore_create_device(c->device, reference, c->exons, params, c->pairs.p, c->n_pairs, c->n_seq_names, out);
    if (rc) return TASKT_FAIL(rc, "taskt_store_create: %s", task_last_error());
    return DSA_OK;
}

int taskt_get_timing(const taskt_ctx* c, taskt_timing* out)
{
    if (!c || !out) return TASKT_FAIL(DSA_E_ARG, "taskt_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
