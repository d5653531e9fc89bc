// span_api.hip — splitreads.span.stats (scripts/calc_span_stats.pl) on gfx950 from cluster text and break positions in device
// memory (include/defuse_ptext.h, section "span statistics").  What a line, a term and a printed number are stands in
// span_shared.hpp, which a host program compiles too.
//
// Tables (span_breaks_text, span_breaks_pred).  Text: txt_shared.hpp's line and tab tables, then one lane per line applies the
// line rule through the tab table (field 1 of a .seq line is a whole sequence and is never scanned).  Pred: one lane per group
// gives its two break entries and its inter 0, groups without lines a key behind all others.  Either way the entries are
// sorted stably by (id, end) or id with the sign bits turned, the last of each run wins, and an exclusive sum of the winners
// places them: two dense sorted columns per table, which a lane searches by bisection.
// Statistics (span_stats), over the lines of a taskc_ctx where they lie:
//   sort 1   stable, by (id, end): groups and ids are numbered by inclusive sums of their heads; a group's strand is its last
//            line's; an id's ends are the groups between its first and its last line
//   sort 2   stable, by (id, fragment) on the order of sort 1, which leaves a fragment's ends ascending and each end's lines in
//            file order: the last line of every (id, fragment, end) is the winner
//   terms    one lane per line: a winner finds its break, reads the one position field its group's strand selects from the
//            text and gives its int64 term; a fragment's first line adds the id's inter and counts the fragment; what stops
//            the id goes into the id's slot by an integer atomicMin, the first rule of the header lowest
//   sums     two 64-bit inclusive sums; an id's sum and count are differences at its two edges (integers: any order, same bits)
//   rows     one lane per id: the stops of the id as a whole, the mean by one IEEE division, the row's length; exclusive sums
//            give each row its rank and its offset; one lane per row prints it with byte stores
// Every per-line array is indexed below the number of lines, every per-id array below the number of ids, every lookup inside
// its table, every read of a text inside a line, and every store into the output inside the bytes its scan counted.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <string>

#include "../../include/defuse_ptext.h"
#include "hip_host.hpp"
#include "pred_shared.hpp"
#include "span_shared.hpp"
#include "txt_shared.hpp"

// taskc_api.hip
__attribute__((visibility("hidden"))) int taskc_lines_device(taskc_ctx* c, bool from_dedup, taskc_lines_view* out);

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;

thread_local std::string g_span_err;

#define SPAN_HIP(call) HIPHOST_TRY(g_span_err, call)
#define SPAN_FAIL(code, ...) hiphost::fail(g_span_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t SIGN = 0x80000000u;        // int order as unsigned order
constexpr u64 HIGH = 0xFFFFFFFF00000000ull;
constexpr u64 BEHIND = ~0ull;                 // the key of a pred group without lines
static_assert(sizeof(span_result) == 96 && sizeof(span_row) == 40 && sizeof(span_device_view) == 40 && sizeof(span_timing) == 48, "C ABI layout");

// what the host reads between the stages (in: the stops NONE, the counts 0)
struct Summary {
    uint32_t stop_line;         // the lowest line a line rule stopped
    uint32_t bad_row;           // the lowest id (its rank) with a stop
    uint32_t n_ids, pad_;
    u64 n_noncanonical, n_entries, n_rows;
    int64_t out_bytes;
};

// the two tables of a ctx as a kernel takes them
struct Tables {
    const u64* bkey;            // (id, end), ascending, distinct
    const int32_t* bval;
    const u64* ikey;            // id in the high word, ascending, distinct
    const int32_t* ival;
    int64_t nb, ni;
};

__host__ __device__ inline u64 pack(int32_t id, int32_t end) { return ((u64)((uint32_t)id ^ SIGN) << 32) | (u64)((uint32_t)end ^ SIGN); }
__host__ __device__ inline u64 pack_id(int32_t id) { return (u64)((uint32_t)id ^ SIGN) << 32; }
__device__ inline uint32_t hi(u64 k) { return (uint32_t)(k >> 32); }
__device__ inline uint32_t lo(u64 k) { return (uint32_t)k; }

// the first index of the ascending a[0 .. n) that is not below key
__device__ inline int64_t lower_bound(const u64* __restrict__ a, int64_t n, u64 key)
{
    int64_t l = 0, h = n;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (a[mid] < key) l = mid + 1; else h = mid;
    }
    return l;
}

__device__ inline int64_t find(const u64* __restrict__ a, int64_t n, u64 key)
{
    const int64_t k = lower_bound(a, n, key);
    return k < n && a[k] == key ? k : n;
}

__device__ inline bool has_break(const Tables& T, uint32_t idk)
{
    const int64_t k = lower_bound(T.bkey, T.nb, (u64)idk << 32);
    return k < T.nb && hi(T.bkey[k]) == idk;
}

// ---- tables -----------------------------------------------------------------------------------------------------------

// one lane per line of the .break (which 0) or the .seq text
__global__ __launch_bounds__(BLOCK) void k_file_lines(Lines L, int64_t n_lines, int which, u64* __restrict__ key, int32_t* __restrict__ val,
                                                       uint32_t* __restrict__ idx, Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_lines) return;
    const LineAt a = line_at(L, i);
    const TabAt tabs{L.tab_pos + a.t0};
    const span_entry r = which == 0 ? span_break_line(L.text, a.s, a.e, tabs, a.n_tabs, DeviceInt()) : span_seq_line(L.text, a.s, a.e, tabs, a.n_tabs, DeviceInt());
    if (r.kind) atomicMin(&sum->stop_line, (uint32_t)i);                        // (rare)
    if (r.noncanonical) atomicAdd(&sum->n_noncanonical, (u64)r.noncanonical);  // (rare)
    key[i] = which == 0 ? pack(r.id, r.end) : pack_id(r.id);
    val[i] = r.value;
    idx[i] = (uint32_t)i;
}

// entry 2 g + end of group g (which 0), or entry g: the break position its .break line carries, or inter 0
__global__ __launch_bounds__(BLOCK) void k_pred_entries(const pred_result* __restrict__ res, int64_t n, int which, u64* __restrict__ key,
                                                         int32_t* __restrict__ val, uint32_t* __restrict__ idx)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const pred_result r = res[g];
    const bool lines = ptext_has_lines(r.status);
    if (which == 0) {
        for (int end = 0; end < 2; ++end) {
            key[2 * g + end] = lines ? pack(r.fusion_id, end) : BEHIND;
            val[2 * g + end] = lines ? ptext_break_pos(r, end) : 0;
            idx[2 * g + end] = (uint32_t)(2 * g + end);
        }
    } else {
        key[g] = lines ? pack_id(r.fusion_id) : BEHIND;
        val[g] = 0;
        idx[g] = (uint32_t)g;
    }
}

// after the sort: the last of every run of one key (with drop, the run of BEHIND has none)
__global__ __launch_bounds__(BLOCK) void k_run_last(const u64* __restrict__ key, int64_t n, bool drop, uint32_t* __restrict__ flag)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n) flag[s] = ((s + 1 == n || key[s + 1] != key[s]) && !(drop && key[s] == BEHIND)) ? 1u : 0u;
}

__global__ __launch_bounds__(BLOCK) void k_table_place(const u64* __restrict__ key, const uint32_t* __restrict__ idx, const int32_t* __restrict__ val,
                                                        const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, int64_t n, u64* __restrict__ out_key,
                                                        int32_t* __restrict__ out_val, Summary* __restrict__ sum)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    if (s == n - 1) sum->n_entries = (u64)rank[s] + (u64)flag[s];
    const int64_t i = idx[s], j = rank[s];                                      // j below the number of winners, which is at most n
    if (!flag[s] || i >= n || j >= n) return;
    out_key[j] = key[s];
    out_val[j] = val[i];
}

// ---- statistics -------------------------------------------------------------------------------------------------------

__device__ inline int64_t source_line(const taskc_lines_view& V, int64_t k) { return V.src ? (int64_t)V.src[k] : k; }

__global__ __launch_bounds__(BLOCK) void k_cluster_keys(taskc_lines_view V, u64* __restrict__ key, uint32_t* __restrict__ idx, Summary* __restrict__ sum)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= V.n_lines) return;
    const int64_t i = source_line(V, k);
    u64 v = 0;
    if (i < V.n_input_lines) {
        const taskc_line r = V.rec[i];
        int field;
        if (span_cluster_stop(r, field)) {
            atomicMin(&sum->stop_line, (uint32_t)k);                            // (rare)
        } else {
            const int64_t s = V.lstart[i];
            const int32_t nc = span_cluster_noncanonical(V.text, s, s + (int64_t)V.llen[i], DeviceInt());
            if (nc) atomicAdd(&sum->n_noncanonical, (u64)nc);                   // (rare)
        }
        v = pack(r.id, r.ce);
    }
    key[k] = v;
    idx[k] = (uint32_t)k;
}

// where the whole key changes, and where its high word does
__global__ __launch_bounds__(BLOCK) void k_heads(const u64* __restrict__ key, int64_t n, uint32_t* __restrict__ head, uint32_t* __restrict__ id_head)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n) return;
    head[s] = (s == 0 || key[s] != key[s - 1]) ? 1u : 0u;
    id_head[s] = (s == 0 || hi(key[s]) != hi(key[s - 1])) ? 1u : 0u;
}

// in the order of sort 1: a group's strand from its last line, the groups at an id's two edges, and the keys of sort 2
__global__ __launch_bounds__(BLOCK) void k_groups(const u64* __restrict__ key, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ gp,
                                                   const uint32_t* __restrict__ ir, taskc_lines_view V, uint8_t* __restrict__ gplus, uint32_t* __restrict__ head_gp,
                                                   uint32_t* __restrict__ tail_gp, u64* __restrict__ key2, uint32_t* __restrict__ val2)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x, q = V.n_lines;
    if (s >= q) return;
    const int64_t k = idx[s];
    const int64_t i = k < q ? source_line(V, k) : V.n_input_lines;
    const int64_t g = (int64_t)gp[s] - 1, r = (int64_t)ir[s] - 1;               // in [0, q)
    int32_t frag = 0;
    if (i < V.n_input_lines && g >= 0 && g < q && r >= 0 && r < q) {
        const taskc_line rec = V.rec[i];
        frag = rec.frag;
        if (s + 1 == q || key[s + 1] != key[s]) gplus[g] = span_is_plus(rec, V.text, V.lstart[i]) ? 1 : 0;
        if (s == 0 || hi(key[s - 1]) != hi(key[s])) head_gp[r] = gp[s];
        if (s + 1 == q || hi(key[s + 1]) != hi(key[s])) tail_gp[r] = gp[s];
    }
    key2[s] = (key[s] & HIGH) | (u64)((uint32_t)frag ^ SIGN);
    val2[s] = (uint32_t)s;
}

// in the order of sort 2 (key2, val2 = the place in sort 1): see the head of the file.  id_stop in: NONE.
__global__ __launch_bounds__(BLOCK) void k_terms(const u64* __restrict__ key2, const uint32_t* __restrict__ val2, const u64* __restrict__ key1,
                                                  const uint32_t* __restrict__ idx1, const uint32_t* __restrict__ gp, const uint8_t* __restrict__ gplus,
                                                  const uint32_t* __restrict__ frag_head, const uint32_t* __restrict__ ir, taskc_lines_view V, Tables T,
                                                  int64_t* __restrict__ term, int64_t* __restrict__ cnt, uint32_t* __restrict__ head_pos,
                                                  uint32_t* __restrict__ tail_pos, uint32_t* __restrict__ id_stop, Summary* __restrict__ sum)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x, q = V.n_lines;
    if (t >= q) return;
    int64_t v = 0;
    uint32_t fh = 0;
    const int64_t s1 = val2[t], r = (int64_t)ir[t] - 1;
    if (s1 < q && r >= 0 && r < q) {
        const uint32_t idk = hi(key2[t]), endk = lo(key1[s1]);
        if (t == 0 || hi(key2[t - 1]) != idk) head_pos[r] = (uint32_t)t;
        if (t + 1 == q || hi(key2[t + 1]) != idk) tail_pos[r] = (uint32_t)t;
        if (t + 1 == q) sum->n_ids = ir[t];
        fh = frag_head[t];
        const int64_t k = idx1[s1];
        const int64_t i = k < q ? source_line(V, k) : V.n_input_lines;
        const int64_t g = (int64_t)gp[s1] - 1;
        if (i < V.n_input_lines && g >= 0 && g < q && has_break(T, idk)) {
            uint32_t stop = NONE;
            bool winner = t + 1 == q || key2[t + 1] != key2[t];
            if (!winner) {
                const int64_t n1 = val2[t + 1];
                winner = n1 >= q || lo(key1[n1]) != endk;
            }
            if (winner) {
                const bool plus = gplus[g] != 0;
                const int64_t b = find(T.bkey, T.nb, ((u64)idk << 32) | (u64)endk);
                int32_t brk = 0, pos = 0, field = 0;
                if (b == T.nb) stop = min(stop, 16u * span_stop_rank(SPAN_NO_BREAK_END));
                else if (!span_coord_ok(brk = T.bval[b])) stop = min(stop, 16u * span_stop_rank(SPAN_COORD_LIMIT));
                const int64_t s = V.lstart[i];
                if (!span_position(V.text, s, s + (int64_t)V.llen[i], V.rec[i], plus, DeviceInt(), pos, field))
                    stop = min(stop, 16u * span_stop_rank(SPAN_BAD_INTEGER) + (uint32_t)field);
                else if (!span_coord_ok(pos)) stop = min(stop, 16u * span_stop_rank(SPAN_COORD_LIMIT));
                if (stop == NONE) v = span_term(plus, brk, pos);
            }
            if (fh) {
                const int64_t e = find(T.ikey, T.ni, (u64)idk << 32);
                if (e == T.ni) stop = min(stop, 16u * span_stop_rank(SPAN_NO_INTER));
                else if (!span_coord_ok(T.ival[e])) stop = min(stop, 16u * span_stop_rank(SPAN_COORD_LIMIT));
                else v += (int64_t)T.ival[e];
            }
            if (stop != NONE) atomicMin(&id_stop[r], stop);                     // (rare)
        }
    }
    term[t] = v;
    cnt[t] = (int64_t)fh;
}

// one lane per id
__global__ __launch_bounds__(BLOCK) void k_rows(const uint32_t* __restrict__ head_pos, const uint32_t* __restrict__ tail_pos, const uint32_t* __restrict__ head_gp,
                                                 const uint32_t* __restrict__ tail_gp, const int64_t* __restrict__ pterm, const int64_t* __restrict__ pcnt,
                                                 const u64* __restrict__ key2, Tables T, int64_t n_ids, int64_t q, uint32_t* __restrict__ id_stop,
                                                 int32_t* __restrict__ rid, int64_t* __restrict__ rsum, int64_t* __restrict__ rcnt, uint32_t* __restrict__ rflag,
                                                 u64* __restrict__ rlen, Summary* __restrict__ sum)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_ids) return;
    const int64_t a = head_pos[r], b = tail_pos[r];
    uint32_t flag = 0;
    u64 len = 0;
    if (a <= b && b < q) {
        const uint32_t idk = hi(key2[a]);
        const int32_t id = (int32_t)(idk ^ SIGN);
        rid[r] = id;
        if (has_break(T, idk)) {
            uint32_t stop = id_stop[r];
            if (tail_gp[r] - head_gp[r] != 1u) stop = min(stop, 16u * span_stop_rank(SPAN_NOT_TWO_ENDS));
            const int64_t s = pterm[b] - (a ? pterm[a - 1] : 0), c = pcnt[b] - (a ? pcnt[a - 1] : 0);
            if (stop == NONE && (!span_sum_ok(s) || c < 1)) stop = 16u * span_stop_rank(SPAN_SUM_LIMIT);
            id_stop[r] = stop;
            rsum[r] = s;
            rcnt[r] = c;
            if (stop != NONE) {
                atomicMin(&sum->bad_row, (uint32_t)r);                          // (rare)
            } else {
                flag = 1;
                len = (u64)span_row_length(id, span_g_of(span_mean(s, c)), c);
            }
        }
    }
    rflag[r] = flag;
    rlen[r] = len;
}

__global__ void k_row_totals(const uint32_t* __restrict__ rflag, const uint32_t* __restrict__ rrank, const u64* __restrict__ rlen, const u64* __restrict__ roff,
                             int64_t n_ids, Summary* __restrict__ sum)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sum->n_rows = (u64)rrank[n_ids - 1] + (u64)rflag[n_ids - 1];
        sum->out_bytes = (int64_t)(roff[n_ids - 1] + rlen[n_ids - 1]);
    }
}

__global__ __launch_bounds__(BLOCK) void k_print(const uint32_t* __restrict__ rflag, const uint32_t* __restrict__ rrank, const u64* __restrict__ rlen,
                                                  const u64* __restrict__ roff, const int32_t* __restrict__ rid, const int64_t* __restrict__ rsum,
                                                  const int64_t* __restrict__ rcnt, int64_t n_ids, span_row* __restrict__ rows, int64_t n_rows,
                                                  uint8_t* __restrict__ text, int64_t text_len)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_ids || !rflag[r]) return;
    const int64_t j = rrank[r], off = (int64_t)roff[r], len = (int64_t)rlen[r];
    if (j >= n_rows || off < 0 || off + len > text_len) return;
    const double mean = span_mean(rsum[r], rcnt[r]);
    const span_g g = span_g_of(mean);
    if ((int64_t)span_row_length(rid[r], g, rcnt[r]) != len) return;
    rows[j] = span_row{rid[r], (int32_t)len, off, rcnt[r], rsum[r], mean};
    span_row_write(rid[r], g, rcnt[r], text + off);
}

// span_format_doubles: the lengths, and after their sum the texts
__global__ __launch_bounds__(BLOCK) void k_g_lengths(const double* __restrict__ x, int64_t n, u64* __restrict__ len, int32_t* __restrict__ len32)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const int l = span_g_length(span_g_of(x[k]));
    len[k] = (u64)l;
    len32[k] = l;
}

__global__ __launch_bounds__(BLOCK) void k_g_write(const double* __restrict__ x, int64_t n, const u64* __restrict__ off, uint8_t* __restrict__ out, int64_t out_len)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const span_g g = span_g_of(x[k]);
    const int64_t o = (int64_t)off[k];
    if (o >= 0 && o + span_g_length(g) <= out_len) span_g_write(g, out + o);
}

}  // namespace

struct __attribute__((visibility("hidden"))) span_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[12];      // 0-3 a file or a pred pass; 4-7 statistics; 8, 9 a fetch
    span_timing timing{};
    // a file's text and tables
    DeviceBuffer<uint8_t, GrowSize> text;
    TextScratch scratch;
    TextTables lines;
    // the two tables
    DeviceBuffer<u64, GrowSize> bkey, ikey;
    DeviceBuffer<int32_t, GrowSize> bval, ival;
    int64_t nb = 0, ni = 0;
    bool has_tables = false;
    // scratch
    DeviceBuffer<Summary> sum;
    Summary h_sum{};
    DeviceBuffer<u64, GrowSize> k64[3], rlen, roff;
    DeviceBuffer<uint32_t, GrowSize> idx[3], flag, rank, head, id_head, gp, ir, head_gp, tail_gp, head_pos, tail_pos, id_stop, rflag, rrank;
    DeviceBuffer<int32_t, GrowSize> val, rid;
    DeviceBuffer<int64_t, GrowSize> term, cnt, pterm, pcnt, rsum, rcnt;
    DeviceBuffer<uint8_t, GrowSize> gplus;
    // the output
    DeviceBuffer<span_row, GrowSize> rows;
    DeviceBuffer<uint8_t, GrowSize> out;
    int64_t n_rows = 0, out_bytes = 0;
    bool has_rows = false;
    uint32_t h_u32 = 0;
    int32_t h_i32 = 0;
};

namespace {

// field_int of txt_shared.hpp and a line's tabs for the host, which reads a stopping line of the caller's text again
struct HostInt {
    bool operator()(const uint8_t* p, int64_t n, int& v) const
    {
        if (n <= 0) return false;
        int64_t k = (p[0] == '+' || p[0] == '-') ? 1 : 0;
        if (k == n) return false;
        long long a = 0;
        for (; k < n; ++k) {
            if (p[k] < '0' || p[k] > '9') return false;
            a = a * 10 + (p[k] - '0');
            if (a > 2147483648LL) return false;
        }
        if (p[0] == '-') a = -a;
        if (a > 2147483647LL || a < -2147483648LL) return false;
        v = (int)a;
        return true;
    }
};

struct HostTabs {
    const int64_t* at;
    int64_t operator()(int64_t k) const { return at[k]; }
};

span_result blank_result()
{
    span_result r{};
    r.stop_field = -1;
    return r;
}

int reset_summary(span_ctx* c)
{
    c->h_sum = Summary{};
    c->h_sum.stop_line = c->h_sum.bad_row = NONE;
    SPAN_HIP(hipMemcpyAsync(c->sum.p, &c->h_sum, sizeof(Summary), hipMemcpyHostToDevice, c->st));
    return DSA_OK;
}

int read_summary(span_ctx* c)
{
    SPAN_HIP(hipMemcpyAsync(&c->h_sum, c->sum.p, sizeof(Summary), hipMemcpyDeviceToHost, c->st));
    SPAN_HIP(hipStreamSynchronize(c->st));
    SPAN_HIP(hipGetLastError());
    return DSA_OK;
}

template <class T>
hipError_t inclusive_sum(span_ctx* c, const T* in, T* out, int64_t n)
{
    return hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, in, out, (int)n, (hipStream_t)c->st); });
}

template <class T>
hipError_t exclusive_sum(span_ctx* c, const T* in, T* out, int64_t n)
{
    return hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, in, out, (int)n, (hipStream_t)c->st); });
}

hipError_t sort_pairs(span_ctx* c, const u64* kin, u64* kout, const uint32_t* vin, uint32_t* vout, int64_t n)
{
    return hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceRadixSort::SortPairs(w, wb, kin, kout, vin, vout, (int)n, 0, 64, (hipStream_t)c->st); });
}

int reserve_entries(span_ctx* c, int64_t n)
{
    for (auto* b : {&c->k64[0], &c->k64[1]}) SPAN_HIP(b->reserve((size_t)n));
    for (auto* b : {&c->idx[0], &c->idx[1], &c->flag, &c->rank}) SPAN_HIP(b->reserve((size_t)n));
    SPAN_HIP(c->val.reserve((size_t)n));
    return DSA_OK;
}

// The n > 0 entries in k64[0] / val / idx[0] into a table: sorted, the last of every key.  The summary is read: n_entries.
int build_table(span_ctx* c, int64_t n, bool drop, DeviceBuffer<u64, GrowSize>& out_key, DeviceBuffer<int32_t, GrowSize>& out_val, int64_t* count)
{
    hipStream_t st = c->st;
    SPAN_HIP(out_key.reserve((size_t)n));
    SPAN_HIP(out_val.reserve((size_t)n));
    SPAN_HIP(sort_pairs(c, c->k64[0].p, c->k64[1].p, c->idx[0].p, c->idx[1].p, n));
    hipLaunchKernelGGL(k_run_last, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, n, drop, c->flag.p);
    SPAN_HIP(exclusive_sum(c, (const uint32_t*)c->flag.p, c->rank.p, n));
    hipLaunchKernelGGL(k_table_place, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, (const uint32_t*)c->idx[1].p, (const int32_t*)c->val.p,
                       (const uint32_t*)c->flag.p, (const uint32_t*)c->rank.p, n, out_key.p, out_val.p, c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    if ((int64_t)c->h_sum.n_entries > n) return SPAN_FAIL(DSA_E_DEVICE, "internal: %llu table entries of %lld", c->h_sum.n_entries, (long long)n);
    *count = (int64_t)c->h_sum.n_entries;
    return DSA_OK;
}

// One of the two files: up, lines, table.  A stop fills r and leaves *stopped true.
int file_table(span_ctx* c, int which, const uint8_t* text, int64_t len, span_result* r, bool* stopped)
{
    hipStream_t st = c->st;
    int64_t& count = which == 0 ? c->nb : c->ni;
    count = 0;
    if (len == 0) return DSA_OK;
    SPAN_HIP(c->text.reserve(padded_size(len)));
    Totals tot{};
    if (const int rc = text_upload_count<true>(g_span_err, c->scratch, c->text.p, text, hipMemcpyHostToDevice, len, c->ev[0], c->ev[1], st, tot)) return rc;
    const int64_t n_lines = (int64_t)tot.n_nl + (tot.last != '\n' ? 1 : 0);
    (which == 0 ? r->n_lines : r->n_seq_lines) = n_lines;
    SPAN_HIP(c->lines.reserve(tot));
    if (const int rc = reserve_entries(c, n_lines)) return rc;
    if (const int rc = reset_summary(c)) return rc;
    const Lines L = c->lines.place<true>(c->scratch, c->text.p, len, tot, st);
    hipLaunchKernelGGL(k_file_lines, dim3(grid_of(n_lines)), dim3(BLOCK), 0, st, L, n_lines, which, c->k64[0].p, c->val.p, c->idx[0].p, c->sum.p);
    SPAN_HIP(hipEventRecord(c->ev[2], st));
    if (const int rc = read_summary(c)) return rc;
    c->timing.upload_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.lines_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
    r->n_noncanonical += (int64_t)c->h_sum.n_noncanonical;
    if ((int64_t)c->h_sum.stop_line < n_lines) {
        // the line again on the host, for its kind and field: the caller's text is at hand
        const int64_t i = c->h_sum.stop_line;
        uint32_t nl[2] = {0, 0};
        if (i > 0) SPAN_HIP(hipMemcpyAsync(&nl[0], c->lines.nl_pos.p + (i - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (i < (int64_t)tot.n_nl) SPAN_HIP(hipMemcpyAsync(&nl[1], c->lines.nl_pos.p + i, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipStreamSynchronize(st));
        const int64_t s = i > 0 ? (int64_t)nl[0] + 1 : 0, e = i < (int64_t)tot.n_nl ? (int64_t)nl[1] : len;
        if (s < 0 || e < s || e > len) return SPAN_FAIL(DSA_E_DEVICE, "internal: line %lld at bytes %lld to %lld of %lld", (long long)(i + 1), (long long)s, (long long)e, (long long)len);
        int64_t tabs[5], n_tabs = 0;
        for (int64_t p = s; p < e && n_tabs < 5; ++p)
            if (text[p] == '\t') tabs[n_tabs++] = p;
        const HostTabs tab{tabs};
        const span_entry en = which == 0 ? span_break_line(text, s, e, tab, n_tabs, HostInt()) : span_seq_line(text, s, e, tab, n_tabs, HostInt());
        if (!en.kind) return SPAN_FAIL(DSA_E_DEVICE, "internal: a stop at line %lld that is none", (long long)(i + 1));
        r->stop_line = i + 1;
        r->stop_kind = en.kind;
        r->stop_field = en.field;
        r->stop_file = which == 0 ? SPAN_FILE_BREAKS : SPAN_FILE_SEQS;
        *stopped = true;
        return DSA_OK;
    }
    if (const int rc = build_table(c, n_lines, false, which == 0 ? c->bkey : c->ikey, which == 0 ? c->bval : c->ival, &count)) return rc;
    SPAN_HIP(hipEventRecord(c->ev[3], st));
    SPAN_HIP(hipStreamSynchronize(st));
    c->timing.tables_ms += hiphost::elapsed(c->ev[2], c->ev[3]);
    return DSA_OK;
}

int pred_tables(span_ctx* c, const pred_ctx* p, span_result* r)
{
    hipStream_t st = c->st;
    const int64_t n = p->n_results;
    r->n_lines = n;
    c->nb = c->ni = 0;
    if (n == 0) return DSA_OK;
    if (n > (int64_t)INT32_MAX / 2) return SPAN_FAIL(DSA_E_LIMIT, "span_breaks_pred: more than 2^30 - 1 groups");
    if (const int rc = reserve_entries(c, 2 * n)) return rc;
    for (int which = 0; which < 2; ++which) {
        const int64_t m = which == 0 ? 2 * n : n;
        if (const int rc = reset_summary(c)) return rc;
        SPAN_HIP(hipEventRecord(c->ev[0], st));
        hipLaunchKernelGGL(k_pred_entries, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const pred_result*)p->results.p, n, which, c->k64[0].p, c->val.p, c->idx[0].p);
        SPAN_HIP(hipEventRecord(c->ev[1], st));
        if (const int rc = build_table(c, m, true, which == 0 ? c->bkey : c->ikey, which == 0 ? c->bval : c->ival, which == 0 ? &c->nb : &c->ni)) return rc;
        SPAN_HIP(hipEventRecord(c->ev[2], st));
        SPAN_HIP(hipStreamSynchronize(st));
        c->timing.lines_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
        c->timing.tables_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
    }
    return DSA_OK;
}

int stats_run(span_ctx* c, const taskc_lines_view& V, span_result* r)
{
    hipStream_t st = c->st;
    const int64_t q = V.n_lines;
    r->n_lines = q;
    c->timing.n_lines = q;
    if (q == 0) {
        c->has_rows = true;
        return DSA_OK;
    }
    const Tables T{c->bkey.p, c->bval.p, c->ikey.p, c->ival.p, c->nb, c->ni};
    for (auto* b : {&c->k64[0], &c->k64[1], &c->k64[2], &c->rlen, &c->roff}) SPAN_HIP(b->reserve((size_t)q));
    for (auto* b : {&c->idx[0], &c->idx[1], &c->idx[2], &c->head, &c->id_head, &c->gp, &c->ir, &c->head_gp, &c->tail_gp, &c->head_pos, &c->tail_pos, &c->id_stop,
                    &c->rflag, &c->rrank})
        SPAN_HIP(b->reserve((size_t)q));
    for (auto* b : {&c->term, &c->cnt, &c->pterm, &c->pcnt, &c->rsum, &c->rcnt}) SPAN_HIP(b->reserve((size_t)q));
    SPAN_HIP(c->rid.reserve((size_t)q));
    SPAN_HIP(c->gplus.reserve((size_t)q));
    if (const int rc = reset_summary(c)) return rc;
    SPAN_HIP(hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(k_cluster_keys, dim3(grid_of(q)), dim3(BLOCK), 0, st, V, c->k64[0].p, c->idx[0].p, c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    r->n_noncanonical = (int64_t)c->h_sum.n_noncanonical;
    if ((int64_t)c->h_sum.stop_line < q) {
        const int64_t k = c->h_sum.stop_line;
        int64_t i = k;
        if (V.src) {
            SPAN_HIP(hipMemcpyAsync(&c->h_u32, V.src + k, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            SPAN_HIP(hipStreamSynchronize(st));
            i = c->h_u32;
        }
        if (i >= V.n_input_lines) return SPAN_FAIL(DSA_E_DEVICE, "internal: line %lld of the source is input line %lld of %lld", (long long)k, (long long)i, (long long)V.n_input_lines);
        taskc_line rec{};
        SPAN_HIP(hipMemcpyAsync(&rec, V.rec + i, sizeof rec, hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipStreamSynchronize(st));
        int field = -1;
        r->stop_kind = span_cluster_stop(rec, field);
        if (!r->stop_kind) return SPAN_FAIL(DSA_E_DEVICE, "internal: a stop at line %lld that is none", (long long)(k + 1));
        r->stop_field = field;
        r->stop_line = k + 1;
        r->stop_file = SPAN_FILE_CLUSTERS;
        return DSA_OK;
    }
    u64 *key1 = c->k64[1].p, *key2 = c->k64[2].p;
    uint32_t *idx1 = c->idx[1].p, *val2 = c->idx[2].p;
    // sort 1, groups and ids
    SPAN_HIP(sort_pairs(c, c->k64[0].p, key1, c->idx[0].p, idx1, q));
    hipLaunchKernelGGL(k_heads, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)key1, q, c->head.p, c->id_head.p);
    SPAN_HIP(inclusive_sum(c, (const uint32_t*)c->head.p, c->gp.p, q));
    SPAN_HIP(inclusive_sum(c, (const uint32_t*)c->id_head.p, c->ir.p, q));
    hipLaunchKernelGGL(k_groups, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)key1, (const uint32_t*)idx1, (const uint32_t*)c->gp.p, (const uint32_t*)c->ir.p, V,
                       c->gplus.p, c->head_gp.p, c->tail_gp.p, c->k64[0].p, c->idx[0].p);
    // sort 2; the ids have the ranks they had
    SPAN_HIP(sort_pairs(c, c->k64[0].p, key2, c->idx[0].p, val2, q));
    hipLaunchKernelGGL(k_heads, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)key2, q, c->head.p, c->id_head.p);
    SPAN_HIP(inclusive_sum(c, (const uint32_t*)c->id_head.p, c->ir.p, q));
    SPAN_HIP(hipEventRecord(c->ev[5], st));
    // terms and sums
    SPAN_HIP(hipMemsetAsync(c->id_stop.p, 0xFF, (size_t)q * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_terms, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)key2, (const uint32_t*)val2, (const u64*)key1, (const uint32_t*)idx1,
                       (const uint32_t*)c->gp.p, (const uint8_t*)c->gplus.p, (const uint32_t*)c->head.p, (const uint32_t*)c->ir.p, V, T, c->term.p, c->cnt.p,
                       c->head_pos.p, c->tail_pos.p, c->id_stop.p, c->sum.p);
    SPAN_HIP(inclusive_sum(c, (const int64_t*)c->term.p, c->pterm.p, q));
    SPAN_HIP(inclusive_sum(c, (const int64_t*)c->cnt.p, c->pcnt.p, q));
    if (const int rc = read_summary(c)) return rc;
    const int64_t n_ids = c->h_sum.n_ids;
    if (n_ids < 1 || n_ids > q) return SPAN_FAIL(DSA_E_DEVICE, "internal: %lld ids of %lld lines", (long long)n_ids, (long long)q);
    hipLaunchKernelGGL(k_rows, dim3(grid_of(n_ids)), dim3(BLOCK), 0, st, (const uint32_t*)c->head_pos.p, (const uint32_t*)c->tail_pos.p, (const uint32_t*)c->head_gp.p,
                       (const uint32_t*)c->tail_gp.p, (const int64_t*)c->pterm.p, (const int64_t*)c->pcnt.p, (const u64*)key2, T, n_ids, q, c->id_stop.p, c->rid.p,
                       c->rsum.p, c->rcnt.p, c->rflag.p, c->rlen.p, c->sum.p);
    SPAN_HIP(hipEventRecord(c->ev[6], st));
    // offsets, rows, text
    SPAN_HIP(exclusive_sum(c, (const uint32_t*)c->rflag.p, c->rrank.p, n_ids));
    SPAN_HIP(exclusive_sum(c, (const u64*)c->rlen.p, c->roff.p, n_ids));
    hipLaunchKernelGGL(k_row_totals, dim3(1), dim3(64), 0, st, (const uint32_t*)c->rflag.p, (const uint32_t*)c->rrank.p, (const u64*)c->rlen.p, (const u64*)c->roff.p,
                       n_ids, c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    r->n_ids = n_ids;
    if ((int64_t)c->h_sum.bad_row < n_ids) {
        SPAN_HIP(hipMemcpyAsync(&c->h_u32, c->id_stop.p + c->h_sum.bad_row, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipMemcpyAsync(&c->h_i32, c->rid.p + c->h_sum.bad_row, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipStreamSynchronize(st));
        const int rank = (int)(c->h_u32 >> 4);
        if (rank < 1 || rank > 6) return SPAN_FAIL(DSA_E_DEVICE, "internal: a stop of id %d that is none", c->h_i32);
        r->stop_kind = span_stop_kind(rank);
        r->stop_field = r->stop_kind == SPAN_BAD_INTEGER ? (int32_t)(c->h_u32 & 15u) : -1;
        r->stop_value = c->h_i32;
        r->stop_file = SPAN_FILE_CLUSTERS;
        return DSA_OK;
    }
    const int64_t n_rows = (int64_t)c->h_sum.n_rows, out_bytes = c->h_sum.out_bytes;
    if (n_rows > n_ids || out_bytes < 0 || out_bytes > n_rows * (int64_t)(11 + 1 + SPAN_G_MAX + 1 + 20 + 1))
        return SPAN_FAIL(DSA_E_DEVICE, "internal: %lld rows of %lld ids in %lld bytes", (long long)n_rows, (long long)n_ids, (long long)out_bytes);
    SPAN_HIP(c->rows.reserve((size_t)n_rows));
    SPAN_HIP(c->out.reserve((size_t)out_bytes));
    hipLaunchKernelGGL(k_print, dim3(grid_of(n_ids)), dim3(BLOCK), 0, st, (const uint32_t*)c->rflag.p, (const uint32_t*)c->rrank.p, (const u64*)c->rlen.p,
                       (const u64*)c->roff.p, (const int32_t*)c->rid.p, (const int64_t*)c->rsum.p, (const int64_t*)c->rcnt.p, n_ids, c->rows.p, n_rows, c->out.p, out_bytes);
    SPAN_HIP(hipEventRecord(c->ev[7], st));
    SPAN_HIP(hipStreamSynchronize(st));
    SPAN_HIP(hipGetLastError());
    c->timing.sorts_ms = hiphost::elapsed(c->ev[4], c->ev[5]);
    c->timing.terms_ms = hiphost::elapsed(c->ev[5], c->ev[6]);
    c->timing.print_ms = hiphost::elapsed(c->ev[6], c->ev[7]);
    c->timing.n_rows = n_rows;
    c->n_rows = n_rows;
    c->out_bytes = out_bytes;
    c->has_rows = true;
    r->n_rows = n_rows;
    r->out_bytes = out_bytes;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* span_last_error(void) { return g_span_err.c_str(); }

int span_create(int device, span_ctx** out)
{
    if (!out) return SPAN_FAIL(DSA_E_ARG, "span_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_span_err)) return DSA_E_DEVICE;
    SPAN_HIP(hipSetDevice(device));
    span_ctx* c = new span_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    // the tables and the view of an empty output have pointers too
    ok = ok && c->sum.reserve(1) == hipSuccess && c->bkey.reserve(1) == hipSuccess && c->bval.reserve(1) == hipSuccess && c->ikey.reserve(1) == hipSuccess &&
         c->ival.reserve(1) == hipSuccess && c->rows.reserve(1) == hipSuccess && c->out.reserve(1) == hipSuccess;
    if (!ok) {
        delete c;
        return SPAN_FAIL(DSA_E_DEVICE, "span_create: cannot create a stream, an event or a buffer");
    }
    *out = c;
    return DSA_OK;
}

void span_destroy(span_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int span_breaks_text(span_ctx* c, const uint8_t* brk_text, int64_t brk_len, const uint8_t* seq_text, int64_t seq_len, span_result* r)
{
    if (!r) return SPAN_FAIL(DSA_E_ARG, "span_breaks_text: no result");
    *r = blank_result();
    if (brk_len < 0 || seq_len < 0) return SPAN_FAIL(DSA_E_ARG, "span_breaks_text: negative length (%lld, %lld)", (long long)brk_len, (long long)seq_len);
    if (brk_len > (int64_t)INT32_MAX || seq_len > (int64_t)INT32_MAX)
        return SPAN_FAIL(DSA_E_LIMIT, "span_breaks_text: a text of %lld bytes, more than 2^31 - 1", (long long)(brk_len > seq_len ? brk_len : seq_len));
    if ((brk_len && !brk_text) || (seq_len && !seq_text)) return SPAN_FAIL(DSA_E_ARG, "span_breaks_text: null pointer with non-zero size");
    if (!c) return SPAN_FAIL(DSA_E_ARG, "span_breaks_text: no ctx");
    c->has_tables = false;
    c->timing.upload_ms = c->timing.lines_ms = c->timing.tables_ms = 0.f;
    SPAN_HIP(hipSetDevice(c->device));
    bool stopped = false;
    int rc = file_table(c, 0, brk_text, brk_len, r, &stopped);
    if (rc == DSA_OK && !stopped) rc = file_table(c, 1, seq_text, seq_len, r, &stopped);
    if (rc != DSA_OK || stopped) {
        (void)hipStreamSynchronize(c->st);                  // nothing of a refused call is in flight when it returns
        c->nb = c->ni = 0;
        if (rc != DSA_OK) *r = blank_result();
        return rc;
    }
    c->has_tables = true;
    r->n_breaks = c->nb;
    r->n_inters = c->ni;
    return DSA_OK;
}

int span_breaks_pred(span_ctx* c, const pred_ctx* p, span_result* r)
{
    if (!r) return SPAN_FAIL(DSA_E_ARG, "span_breaks_pred: no result");
    *r = blank_result();
    if (!c || !p) return SPAN_FAIL(DSA_E_ARG, "span_breaks_pred: no %s", !c ? "ctx" : "pred ctx");
    c->has_tables = false;
    c->timing.upload_ms = c->timing.lines_ms = c->timing.tables_ms = 0.f;
    if (c->device != p->device) return SPAN_FAIL(DSA_E_ARG, "span_breaks_pred: ctx and pred ctx are on devices %d and %d", c->device, p->device);
    if (!p->predicted) return SPAN_FAIL(DSA_E_ARG, "span_breaks_pred: the pred ctx has no completed prediction (none yet, or its latest call failed)");
    SPAN_HIP(hipSetDevice(c->device));
    const int rc = pred_tables(c, p, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->nb = c->ni = 0;
        *r = blank_result();
        return rc;
    }
    c->has_tables = true;
    r->n_breaks = c->nb;
    r->n_inters = c->ni;
    return DSA_OK;
}

int span_stats(span_ctx* c, taskc_ctx* clusters, int32_t source, span_result* r)
{
    if (!r) return SPAN_FAIL(DSA_E_ARG, "span_stats: no result");
    *r = blank_result();
    if (source != TASKC_INPUT && source != TASKC_DEDUP) return SPAN_FAIL(DSA_E_ARG, "span_stats: source %d is neither TASKC_INPUT nor TASKC_DEDUP", source);
    if (!c || !clusters) return SPAN_FAIL(DSA_E_ARG, "span_stats: no %s", !c ? "ctx" : "cluster ctx");
    c->has_rows = false;
    c->n_rows = c->out_bytes = 0;
    c->timing.sorts_ms = c->timing.terms_ms = c->timing.print_ms = c->timing.download_ms = 0.f;
    c->timing.n_lines = c->timing.n_rows = 0;
    if (!c->has_tables) return SPAN_FAIL(DSA_E_ARG, "span_stats: the ctx has no tables (span_breaks_text or span_breaks_pred first)");
    taskc_lines_view V{};
    if (const int rc = taskc_lines_device(clusters, source == TASKC_DEDUP, &V)) return SPAN_FAIL(rc, "span_stats: %s", taskc_last_error());
    if (V.device != c->device) return SPAN_FAIL(DSA_E_ARG, "span_stats: ctx and cluster ctx are on devices %d and %d", c->device, V.device);
    SPAN_HIP(hipSetDevice(c->device));
    const int rc = stats_run(c, V, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->has_rows = false;
        *r = blank_result();
    } else if (r->stop_kind) (void)hipStreamSynchronize(c->st);
    return rc;
}

int span_view(const span_ctx* c, span_device_view* out)
{
    if (!c || !out) return SPAN_FAIL(DSA_E_ARG, "span_view: no %s", !c ? "ctx" : "output");
    if (!c->has_rows) return SPAN_FAIL(DSA_E_ARG, "span_view: the ctx has no output (span_stats first)");
    *out = span_device_view{c->rows.p, c->out.p, c->n_rows, c->out_bytes, c->device, 0};
    return DSA_OK;
}

int span_fetch(span_ctx* c, span_row* rows, int64_t rows_cap, uint8_t* text, int64_t text_cap)
{
    if (!c) return SPAN_FAIL(DSA_E_ARG, "span_fetch: no ctx");
    if (rows_cap < 0 || text_cap < 0) return SPAN_FAIL(DSA_E_ARG, "span_fetch: negative capacity");
    if ((rows_cap && !rows) || (text_cap && !text)) return SPAN_FAIL(DSA_E_ARG, "span_fetch: capacity without a buffer");
    if (!c->has_rows) return SPAN_FAIL(DSA_E_ARG, "span_fetch: the ctx has no output (span_stats first)");
    if (rows_cap < c->n_rows || text_cap < c->out_bytes) return SPAN_FAIL(DSA_E_CAPACITY, "the ctx has %lld rows and %lld text bytes", (long long)c->n_rows, (long long)c->out_bytes);
    SPAN_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    SPAN_HIP(hipEventRecord(c->ev[8], st));
    if (c->n_rows) SPAN_HIP(hipMemcpyAsync(rows, c->rows.p, (size_t)c->n_rows * sizeof(span_row), hipMemcpyDeviceToHost, st));
    if (c->out_bytes) SPAN_HIP(hipMemcpyAsync(text, c->out.p, (size_t)c->out_bytes, hipMemcpyDeviceToHost, st));
    SPAN_HIP(hipEventRecord(c->ev[9], st));
    SPAN_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[8], c->ev[9]);
    return DSA_OK;
}

int span_get_timing(const span_ctx* c, span_timing* out)
{
    if (!c || !out) return SPAN_FAIL(DSA_E_ARG, "span_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

int span_format_doubles(int device, const double* x, int64_t n, uint8_t* out, int64_t cap, int32_t* len, int64_t* out_len)
{
    if (!out_len) return SPAN_FAIL(DSA_E_ARG, "span_format_doubles: no output length");
    *out_len = 0;
    if (n < 0 || cap < 0) return SPAN_FAIL(DSA_E_ARG, "span_format_doubles: negative size (%lld values, capacity %lld)", (long long)n, (long long)cap);
    if (n > (int64_t)INT32_MAX / 2) return SPAN_FAIL(DSA_E_LIMIT, "span_format_doubles: more than 2^30 - 1 values in one call");
    if ((n && (!x || !len)) || (cap && !out)) return SPAN_FAIL(DSA_E_ARG, "span_format_doubles: null pointer with non-zero size");
    if (hiphost::check_device(device, &g_span_err)) return DSA_E_DEVICE;
    if (n == 0) return DSA_OK;
    SPAN_HIP(hipSetDevice(device));
    hiphost::Stream stream;
    DeviceBuffer<double> dx;
    DeviceBuffer<u64> dlen, doff;
    DeviceBuffer<int32_t> dlen32;
    DeviceBuffer<uint8_t> dout;
    DeviceBuffer<uint8_t, GrowSize> tmp;
    SPAN_HIP(stream.create(hipStreamNonBlocking));
    hipStream_t st = stream;
    auto run = [&]() -> int {
        SPAN_HIP(dx.reserve((size_t)n));
        SPAN_HIP(dlen.reserve((size_t)n));
        SPAN_HIP(doff.reserve((size_t)n));
        SPAN_HIP(dlen32.reserve((size_t)n));
        SPAN_HIP(hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_g_lengths, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const double*)dx.p, n, dlen.p, dlen32.p);
        SPAN_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, dlen.p, doff.p, (int)n, st); }));
        u64 last[2] = {0, 0};
        SPAN_HIP(hipMemcpyAsync(&last[0], doff.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipMemcpyAsync(&last[1], dlen.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipStreamSynchronize(st));
        SPAN_HIP(hipGetLastError());
        const u64 total = last[0] + last[1];
        if (total > (u64)n * (u64)SPAN_G_MAX) return SPAN_FAIL(DSA_E_DEVICE, "internal: %llu text bytes of %lld values", total, (long long)n);
        *out_len = (int64_t)total;
        if ((int64_t)total > cap) return SPAN_FAIL(DSA_E_CAPACITY, "the texts have %llu bytes", total);
        SPAN_HIP(dout.reserve((size_t)total));
        hipLaunchKernelGGL(k_g_write, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const double*)dx.p, n, (const u64*)doff.p, dout.p, (int64_t)total);
        if (total) SPAN_HIP(hipMemcpyAsync(out, dout.p, (size_t)total, hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipMemcpyAsync(len, dlen32.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SPAN_HIP(hipStreamSynchronize(st));
        SPAN_HIP(hipGetLastError());
        return DSA_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);                           // nothing is in flight when the buffers go
    return rc;
}

}  // extern "C"
