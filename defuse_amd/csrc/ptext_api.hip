// ptext_api.hip — WriteSequence and WriteBreak (tools/SplitAlignment.cpp:596-615) for all groups of a prediction on gfx950
// (include/defuse_ptext.h): the bytes of splitreads.seq and splitreads.break, from the results and the sequences that
// pred_predict* left on the device.  What a line is stands in ptext_shared.hpp, which a host program compiles too.
//
// Names (ptext_names_create).  The host looks at every end anyway to refuse a doubled key, so the ends go up sorted by
// (fusion_id as unsigned, cluster_end) in one 64-bit key column, each with its name's offset and length in the name bytes and
// its align strand: a kernel finds an end by binary search.
//
// Format (ptext_format), all on the ctx's stream, one host round trip:
//   (1) lengths: one thread per group finds its two ends, decides which lines the group gets (the status rules of the
//       header) and writes the two lengths and the row's status;
//   (2) two 64-bit exclusive sums give the offsets; the two totals and the lowest group with an end that has no entry
//       come back in one small copy and size the texts;
//   (3) write: one thread per group completes its row and writes, with byte stores, the head and the tail of its .seq
//       line, both .break lines, and one copy segment for the sequence between head and tail;
//   (4) the gather (k_bat_gather of bat_shared.hpp, as pred_api.hip uses it) copies the sequences out of the pred_ctx.
// Every byte of either text has one writer and none is written by a read-modify-write: the gather stores a dword only
// where it lies wholly inside its segment and the segment's edge bytes as bytes, and (3) stores bytes only, so the dwords
// that a line's head or tail shares with its sequence, or with a neighbouring line, are never stored to as dwords.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "../../include/defuse_ptext.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "pred_shared.hpp"
#include "ptext_shared.hpp"

namespace {

using batdev::Seg64;
using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using u64 = unsigned long long;

thread_local std::string g_ptext_err;

#define PTEXT_HIP(call) HIPHOST_TRY(g_ptext_err, call)
#define PTEXT_FAIL(code, ...) hiphost::fail(g_ptext_err, code, __VA_ARGS__)

constexpr int BLOCK = batdev::GATHER_BLOCK;
constexpr int SEQ_GROUP = 64;         // lanes per sequence: a few hundred bases and more
constexpr u64 NO_GROUP = ~0ull;

static_assert(sizeof(ptext_end) == 16 && sizeof(ptext_line) == 40 && sizeof(ptext_device_view) == 56 && sizeof(ptext_timing) == 48, "C ABI layout");

// a cluster end on the device
struct DevEnd {
    int64_t name_off;
    int32_t name_len;
    int32_t strand;
};

__host__ __device__ inline u64 end_key(int32_t fusion_id, int end) { return ((u64)(uint32_t)fusion_id << 1) | (u64)end; }

// the index of `key` in the ascending a[0 .. n), n if it is not there
__device__ inline int64_t find_end(const u64* __restrict__ a, int64_t n, u64 key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && a[lo] == key ? lo : n;
}

// head[2]: the lowest group that gets lines and has an end without an entry (NO_GROUP before the launch); head[3]: the
// sequence bytes the gather will copy (0 before the launch), one atomic per workgroup
__global__ __launch_bounds__(BLOCK) void k_ptext_lengths(const pred_result* __restrict__ res, int64_t n, const u64* __restrict__ ekey,
                                                          const DevEnd* __restrict__ dend, int64_t n_ends, u64* __restrict__ len_seq,
                                                          u64* __restrict__ len_brk, ptext_line* __restrict__ lines, u64* __restrict__ head)
{
    using Reduce = hipcub::BlockReduce<u64, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    u64 copied = 0;
    if (g < n) {
        const pred_result r = res[g];
        int64_t ls = 0, lb = 0;
        int32_t status = r.status;
        if (ptext_has_lines(status)) {
            const int64_t e0 = find_end(ekey, n_ends, end_key(r.fusion_id, 0)), e1 = find_end(ekey, n_ends, end_key(r.fusion_id, 1));
            if (e0 == n_ends || e1 == n_ends) {
                atomicMin(&head[2], (u64)g);
            } else {
                lb = (int64_t)ptext_break_length(r, 0, dend[e0].name_len) + ptext_break_length(r, 1, dend[e1].name_len);
                const ptext_seq_parts s = ptext_seq_parts_of(r);
                if (s.ok) {
                    ls = (int64_t)s.head + s.body + s.tail;
                    copied = s.no_split ? 0u : (u64)s.body;
                } else {
                    status |= PTEXT_HOST_SEQ;
                }
            }
        }
        len_seq[g] = (u64)ls;
        len_brk[g] = (u64)lb;
        lines[g] = ptext_line{0, ls, 0, lb, status, 0};
    }
    const u64 sum = Reduce(tmp).Sum(copied);
    if (threadIdx.x == 0 && sum) atomicAdd(&head[3], sum);
}

__global__ void k_ptext_totals(const u64* __restrict__ len_seq, const u64* __restrict__ off_seq, const u64* __restrict__ len_brk,
                               const u64* __restrict__ off_brk, int64_t n, u64* __restrict__ head)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head[0] = off_seq[n - 1] + len_seq[n - 1];
        head[1] = off_brk[n - 1] + len_brk[n - 1];
    }
}

__global__ __launch_bounds__(BLOCK) void k_ptext_write(const pred_result* __restrict__ res, int64_t n, const u64* __restrict__ ekey,
                                                        const DevEnd* __restrict__ dend, int64_t n_ends, const uint8_t* __restrict__ name_bytes,
                                                        const u64* __restrict__ off_seq, const u64* __restrict__ off_brk, ptext_line* __restrict__ lines,
                                                        Seg64* __restrict__ seg, uint8_t* __restrict__ seq_text, int64_t seq_total,
                                                        uint8_t* __restrict__ brk_text, int64_t brk_total)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const pred_result r = res[g];
    ptext_line row = lines[g];
    row.seq_off = (int64_t)off_seq[g];
    row.brk_off = (int64_t)off_brk[g];
    lines[g] = row;
    Seg64 sg{0, 0, 0, 0};
    if (row.seq_len > 0 && row.seq_off >= 0 && row.seq_off + row.seq_len <= seq_total) {
        const ptext_seq_parts s = ptext_seq_parts_of(r);
        uint8_t* out = seq_text + row.seq_off;
        const int head = rec_write_field(r.fusion_id, out);
        if (s.no_split) out[head] = (uint8_t)'N';
        else sg = Seg64{r.seq_off, row.seq_off + head, (uint32_t)s.body, 0};
        ptext_write_seq_tail(s, out + head + s.body);
    }
    if (row.brk_len > 0 && row.brk_off >= 0 && row.brk_off + row.brk_len <= brk_total) {
        uint8_t* out = brk_text + row.brk_off;
        for (int end = 0; end < 2; ++end) {
            const int64_t e = find_end(ekey, n_ends, end_key(r.fusion_id, end));
            if (e == n_ends) break;                                                 // (k_ptext_lengths gave such a group no lines)
            const DevEnd d = dend[e];
            out += ptext_write_break(r, end, name_bytes + d.name_off, d.name_len, d.strand, out);
        }
    }
    seg[g] = sg;
}

// ptext_format_doubles: the lengths, and after their sum the texts
__global__ __launch_bounds__(BLOCK) void k_ptext_g_lengths(const double* __restrict__ x, int64_t n, u64* __restrict__ len, int32_t* __restrict__ len32)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const int l = ptext_g_length(ptext_g_of(x[k]));
    len[k] = (u64)l;
    len32[k] = l;
}

__global__ __launch_bounds__(BLOCK) void k_ptext_g_write(const double* __restrict__ x, int64_t n, const u64* __restrict__ off, uint8_t* __restrict__ out,
                                                          int64_t out_len)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const ptext_g g = ptext_g_of(x[k]);
    const int64_t o = (int64_t)off[k];
    if (o >= 0 && o + ptext_g_length(g) <= out_len) ptext_g_write(g, out + o);
}

}  // namespace

struct __attribute__((visibility("hidden"))) ptext_names {
    int device = -1;
    int64_t n_ends = 0;
    std::vector<u64> keys;                          // the host's copy of ekey: an error names the end that is missing
    hiphost::Stream st;
    DeviceBuffer<uint8_t> bytes;
    DeviceBuffer<u64> ekey;                         // n_ends keys (end_key), ascending, distinct
    DeviceBuffer<DevEnd> dend;                      // in the same order
};

struct __attribute__((visibility("hidden"))) ptext_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[7];       // 0 start, 1 totals on their way, 2 texts sized, 3 written, 4 gathered; 5, 6 around a fetch
    // the texts
    int64_t n_lines = 0, seq_len = 0, brk_len = 0;
    DeviceBuffer<uint8_t, GrowSize> seq_text, brk_text;
    DeviceBuffer<ptext_line, GrowSize> lines;
    // per call
    DeviceBuffer<u64, GrowSize> len_seq, len_brk, off_seq, off_brk;
    DeviceBuffer<u64> head;                         // seq total, break total, lowest group with a missing end, copied bytes
    DeviceBuffer<Seg64, GrowSize> seg;
    DeviceBuffer<uint8_t, GrowSize> tmp;
    ptext_timing timing{};
};

namespace {

int format_on_device(ptext_ctx* c, const pred_ctx* p, const ptext_names* nm, int64_t n)
{
    hipStream_t st = c->st;
    const unsigned gn = grid_of(n);
    const pred_result* res = p->results.p;
    PTEXT_HIP(c->lines.reserve((size_t)n));
    PTEXT_HIP(c->len_seq.reserve((size_t)n));
    PTEXT_HIP(c->len_brk.reserve((size_t)n));
    PTEXT_HIP(c->off_seq.reserve((size_t)n));
    PTEXT_HIP(c->off_brk.reserve((size_t)n));
    PTEXT_HIP(c->seg.reserve((size_t)n));
    PTEXT_HIP(hipEventRecord(c->ev[0], st));
    // (1) lengths
    PTEXT_HIP(hipMemsetAsync(c->head.p, 0, 4 * sizeof(u64), st));
    PTEXT_HIP(hipMemsetAsync(c->head.p + 2, 0xFF, sizeof(u64), st));
    hipLaunchKernelGGL(k_ptext_lengths, dim3(gn), dim3(BLOCK), 0, st, res, n, (const u64*)nm->ekey.p, (const DevEnd*)nm->dend.p, nm->n_ends, c->len_seq.p,
                       c->len_brk.p, c->lines.p, c->head.p);
    // (2) offsets and totals, in 64 bits
    PTEXT_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->len_seq.p, c->off_seq.p, (int)n, st); }));
    PTEXT_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->len_brk.p, c->off_brk.p, (int)n, st); }));
    hipLaunchKernelGGL(k_ptext_totals, dim3(1), dim3(64), 0, st, (const u64*)c->len_seq.p, (const u64*)c->off_seq.p, (const u64*)c->len_brk.p,
                       (const u64*)c->off_brk.p, n, c->head.p);
    u64 head[4] = {0, 0, 0, 0};
    PTEXT_HIP(hipMemcpyAsync(head, c->head.p, sizeof head, hipMemcpyDeviceToHost, st));
    PTEXT_HIP(hipEventRecord(c->ev[1], st));
    PTEXT_HIP(hipStreamSynchronize(st));
    PTEXT_HIP(hipGetLastError());
    if (head[2] != NO_GROUP) {
        pred_result r{};
        if (head[2] >= (u64)n) return PTEXT_FAIL(DSA_E_DEVICE, "internal: group %llu of %lld has no names", head[2], (long long)n);
        PTEXT_HIP(hipMemcpyAsync(&r, res + head[2], sizeof r, hipMemcpyDeviceToHost, st));
        PTEXT_HIP(hipStreamSynchronize(st));
        const int end = std::binary_search(nm->keys.begin(), nm->keys.end(), end_key(r.fusion_id, 0)) ? 1 : 0;
        return PTEXT_FAIL(DSA_E_ARG, "group %llu: cluster end %d of fusion_id %d has no entry in the names", head[2], end, r.fusion_id);
    }
    // a line is at most a sequence of 2^31 - 1 bytes and some hundred more, a name at most 2^31 - 1
    if (head[0] > (u64)n * ((u64)INT32_MAX + 256u) || head[1] > (u64)n * (2u * (u64)INT32_MAX + 256u))
        return PTEXT_FAIL(DSA_E_DEVICE, "internal: %llu and %llu text bytes of %lld groups", head[0], head[1], (long long)n);
    const int64_t ST = (int64_t)head[0], BT = (int64_t)head[1];
    PTEXT_HIP(c->seq_text.reserve((size_t)ST + 4));           // whole dwords
    PTEXT_HIP(c->brk_text.reserve((size_t)BT + 4));
    PTEXT_HIP(hipEventRecord(c->ev[2], st));                  // (a growth of the texts is host time between ev[1] and here)
    // (3) heads, tails, break lines, rows, segments
    hipLaunchKernelGGL(k_ptext_write, dim3(gn), dim3(BLOCK), 0, st, res, n, (const u64*)nm->ekey.p, (const DevEnd*)nm->dend.p, nm->n_ends,
                       (const uint8_t*)nm->bytes.p, (const u64*)c->off_seq.p, (const u64*)c->off_brk.p, c->lines.p, c->seg.p, c->seq_text.p, ST, c->brk_text.p, BT);
    PTEXT_HIP(hipEventRecord(c->ev[3], st));
    // (4) the sequences
    hipLaunchKernelGGL((k_bat_gather<SEQ_GROUP, false, Seg64>), dim3(grid_of(n * SEQ_GROUP)), dim3(BLOCK), 0, st, (const Seg64*)c->seg.p, n,
                       (const uint8_t*)p->seq_bytes.p, p->seq_bytes_len, c->seq_text.p, ST);
    PTEXT_HIP(hipEventRecord(c->ev[4], st));
    PTEXT_HIP(hipStreamSynchronize(st));
    PTEXT_HIP(hipGetLastError());
    c->n_lines = n;
    c->seq_len = ST;
    c->brk_len = BT;
    c->timing.lengths_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.write_ms = hiphost::elapsed(c->ev[2], c->ev[3]);
    c->timing.gather_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    c->timing.seq_text_bytes = ST;
    c->timing.brk_text_bytes = BT;
    c->timing.gather_bytes = (int64_t)head[3];
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* ptext_last_error(void) { return g_ptext_err.c_str(); }

int ptext_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names, const ptext_end* ends,
                       int64_t n_ends, ptext_names** out)
{
    if (!out) return PTEXT_FAIL(DSA_E_ARG, "ptext_names_create: no output");
    *out = nullptr;
    if (n_names < 0 || n_ends < 0 || name_bytes_len < 0)
        return PTEXT_FAIL(DSA_E_ARG, "negative size (%lld names, %lld ends, %lld bytes)", (long long)n_names, (long long)n_ends, (long long)name_bytes_len);
    if (n_names > (int64_t)INT32_MAX || n_ends > (int64_t)INT32_MAX) return PTEXT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 names or ends in one store");
    if ((n_names && !name_off) || (n_ends && !ends) || (name_bytes_len && !name_bytes))
        return PTEXT_FAIL(DSA_E_ARG, "ptext_names_create: null pointer with non-zero size");
    for (int64_t k = 0; k < n_names; ++k) {
        const int64_t a = name_off[k], b = name_off[k + 1];
        if (a < 0 || b < a || b > name_bytes_len)
            return PTEXT_FAIL(DSA_E_ARG, "name %lld: bytes %lld to %lld are negative, reversed or outside the %lld given", (long long)k, (long long)a, (long long)b,
                              (long long)name_bytes_len);
        if (b - a > (int64_t)INT32_MAX) return PTEXT_FAIL(DSA_E_LIMIT, "name %lld: more than 2^31 - 1 bytes", (long long)k);
    }
    std::vector<std::pair<u64, int64_t>> bykey((size_t)n_ends);
    for (int64_t k = 0; k < n_ends; ++k) {
        const ptext_end& e = ends[k];
        if (e.cluster_end != 0 && e.cluster_end != 1) return PTEXT_FAIL(DSA_E_ARG, "end %lld: cluster_end %d is not 0 or 1", (long long)k, e.cluster_end);
        if (e.strand != 0 && e.strand != 1) return PTEXT_FAIL(DSA_E_ARG, "end %lld: strand %d is not 0 or 1", (long long)k, e.strand);
        if (e.name < 0 || (int64_t)e.name >= n_names)
            return PTEXT_FAIL(DSA_E_ARG, "end %lld: name %d is outside the table of %lld", (long long)k, e.name, (long long)n_names);
        bykey[(size_t)k] = {end_key(e.fusion_id, e.cluster_end), k};
    }
    std::sort(bykey.begin(), bykey.end());
    for (int64_t s = 1; s < n_ends; ++s)
        if (bykey[(size_t)s].first == bykey[(size_t)s - 1].first)
            return PTEXT_FAIL(DSA_E_ARG, "ends %lld and %lld: both are cluster end %d of fusion_id %d", (long long)bykey[(size_t)s - 1].second,
                              (long long)bykey[(size_t)s].second, ends[bykey[(size_t)s].second].cluster_end, ends[bykey[(size_t)s].second].fusion_id);
    if (hiphost::check_device(device, &g_ptext_err)) return DSA_E_DEVICE;
    PTEXT_HIP(hipSetDevice(device));
    ptext_names* t = new ptext_names();
    t->device = device;
    t->n_ends = n_ends;
    t->keys.resize((size_t)n_ends);
    std::vector<DevEnd> dend((size_t)n_ends);
    for (int64_t s = 0; s < n_ends; ++s) {
        const ptext_end& e = ends[bykey[(size_t)s].second];
        t->keys[(size_t)s] = bykey[(size_t)s].first;
        dend[(size_t)s] = DevEnd{name_off[e.name], (int32_t)(name_off[e.name + 1] - name_off[e.name]), e.strand};
    }
    auto build = [&]() -> int {
        if (t->st.create(hipStreamNonBlocking) != hipSuccess) return PTEXT_FAIL(DSA_E_DEVICE, "cannot create a stream");
        hipStream_t st = t->st;
        PTEXT_HIP(t->bytes.reserve((size_t)name_bytes_len));
        PTEXT_HIP(t->ekey.reserve((size_t)n_ends));
        PTEXT_HIP(t->dend.reserve((size_t)n_ends));
        if (name_bytes_len) PTEXT_HIP(hipMemcpyAsync(t->bytes.p, name_bytes, (size_t)name_bytes_len, hipMemcpyHostToDevice, st));
        if (n_ends) PTEXT_HIP(hipMemcpyAsync(t->ekey.p, t->keys.data(), (size_t)n_ends * sizeof(u64), hipMemcpyHostToDevice, st));
        if (n_ends) PTEXT_HIP(hipMemcpyAsync(t->dend.p, dend.data(), (size_t)n_ends * sizeof(DevEnd), hipMemcpyHostToDevice, st));
        PTEXT_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    };
    if (const int rc = build()) {
        (void)hipStreamSynchronize(t->st);
        delete t;
        return rc;
    }
    *out = t;
    return DSA_OK;
}

void ptext_names_destroy(ptext_names* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->st);
    delete t;
}

int ptext_create(int device, ptext_ctx** out)
{
    if (!out) return PTEXT_FAIL(DSA_E_ARG, "ptext_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_ptext_err)) return DSA_E_DEVICE;
    PTEXT_HIP(hipSetDevice(device));
    ptext_ctx* c = new ptext_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    // the view of empty texts has pointers too
    ok = ok && c->seq_text.reserve(4) == hipSuccess && c->brk_text.reserve(4) == hipSuccess && c->lines.reserve(1) == hipSuccess &&
         c->head.reserve(4) == hipSuccess;
    if (!ok) {
        delete c;
        return PTEXT_FAIL(DSA_E_DEVICE, "cannot create a stream or a buffer");
    }
    *out = c;
    return DSA_OK;
}

void ptext_destroy(ptext_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int ptext_format(ptext_ctx* c, const pred_ctx* p, const ptext_names* nm)
{
    if (!c || !p || !nm) return PTEXT_FAIL(DSA_E_ARG, "ptext_format: no %s", !c ? "ctx" : !p ? "pred ctx" : "names");
    c->n_lines = c->seq_len = c->brk_len = 0;
    c->timing = ptext_timing{};
    if (c->device != p->device || c->device != nm->device)
        return PTEXT_FAIL(DSA_E_ARG, "ptext_format: ctx, pred ctx and names are on devices %d, %d and %d", c->device, p->device, nm->device);
    if (!p->predicted)
        return PTEXT_FAIL(DSA_E_ARG, "ptext_format: the pred ctx has no completed prediction (none yet, or its latest call failed)");
    const int64_t n = p->n_results;
    c->timing.n_groups = n;
    if (n == 0) return DSA_OK;
    PTEXT_HIP(hipSetDevice(c->device));
    const int rc = format_on_device(c, p, nm, n);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);                  // nothing of a refused call is in flight when it returns
        c->timing = ptext_timing{};
    }
    return rc;
}

int ptext_view(const ptext_ctx* c, ptext_device_view* out)
{
    if (!c || !out) return PTEXT_FAIL(DSA_E_ARG, "ptext_view: no %s", !c ? "ctx" : "output");
    *out = ptext_device_view{c->seq_text.p, c->brk_text.p, c->lines.p, c->seq_len, c->brk_len, c->n_lines, c->device, 0};
    return DSA_OK;
}

int ptext_fetch(ptext_ctx* c, uint8_t* seq_text, int64_t seq_cap, uint8_t* brk_text, int64_t brk_cap, ptext_line* lines, int64_t lines_cap)
{
    if (!c) return PTEXT_FAIL(DSA_E_ARG, "ptext_fetch: no ctx");
    if (seq_cap < 0 || brk_cap < 0 || lines_cap < 0) return PTEXT_FAIL(DSA_E_ARG, "ptext_fetch: negative capacity");
    if ((seq_cap && !seq_text) || (brk_cap && !brk_text) || (lines_cap && !lines)) return PTEXT_FAIL(DSA_E_ARG, "ptext_fetch: capacity without a buffer");
    if (seq_cap < c->seq_len || brk_cap < c->brk_len || lines_cap < c->n_lines)
        return PTEXT_FAIL(DSA_E_CAPACITY, "the ctx has %lld and %lld text bytes and %lld lines", (long long)c->seq_len, (long long)c->brk_len,
                          (long long)c->n_lines);
    PTEXT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    PTEXT_HIP(hipEventRecord(c->ev[5], st));
    if (c->seq_len) PTEXT_HIP(hipMemcpyAsync(seq_text, c->seq_text.p, (size_t)c->seq_len, hipMemcpyDeviceToHost, st));
    if (c->brk_len) PTEXT_HIP(hipMemcpyAsync(brk_text, c->brk_text.p, (size_t)c->brk_len, hipMemcpyDeviceToHost, st));
    if (c->n_lines) PTEXT_HIP(hipMemcpyAsync(lines, c->lines.p, (size_t)c->n_lines * sizeof(ptext_line), hipMemcpyDeviceToHost, st));
    PTEXT_HIP(hipEventRecord(c->ev[6], st));
    PTEXT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[5], c->ev[6]);
    return DSA_OK;
}

int ptext_get_timing(const ptext_ctx* c, ptext_timing* out)
{
    if (!c || !out) return PTEXT_FAIL(DSA_E_ARG, "ptext_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

int ptext_format_doubles(int device, const double* x, int64_t n, uint8_t* out, int64_t cap, int32_t* len, int64_t* out_len)
{
    if (!out_len) return PTEXT_FAIL(DSA_E_ARG, "ptext_format_doubles: no output length");
    *out_len = 0;
    if (n < 0 || cap < 0) return PTEXT_FAIL(DSA_E_ARG, "ptext_format_doubles: negative size (%lld values, capacity %lld)", (long long)n, (long long)cap);
    if (n > (int64_t)INT32_MAX / 2) return PTEXT_FAIL(DSA_E_LIMIT, "ptext_format_doubles: more than 2^30 - 1 values in one call");
    if ((n && (!x || !len)) || (cap && !out)) return PTEXT_FAIL(DSA_E_ARG, "ptext_format_doubles: null pointer with non-zero size");
    if (hiphost::check_device(device, &g_ptext_err)) return DSA_E_DEVICE;
    if (n == 0) return DSA_OK;
    PTEXT_HIP(hipSetDevice(device));
    hiphost::Stream stream;
    DeviceBuffer<double> dx;
    DeviceBuffer<u64> dlen, doff;
    DeviceBuffer<int32_t> dlen32;
    DeviceBuffer<uint8_t> dout;
    DeviceBuffer<uint8_t, GrowSize> tmp;
    PTEXT_HIP(stream.create(hipStreamNonBlocking));
    hipStream_t st = stream;
    auto run = [&]() -> int {
        PTEXT_HIP(dx.reserve((size_t)n));
        PTEXT_HIP(dlen.reserve((size_t)n));
        PTEXT_HIP(doff.reserve((size_t)n));
        PTEXT_HIP(dlen32.reserve((size_t)n));
        PTEXT_HIP(hipMemcpyAsync(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_ptext_g_lengths, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const double*)dx.p, n, dlen.p, dlen32.p);
        PTEXT_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, dlen.p, doff.p, (int)n, st); }));
        u64 last[2] = {0, 0};
        PTEXT_HIP(hipMemcpyAsync(&last[0], doff.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        PTEXT_HIP(hipMemcpyAsync(&last[1], dlen.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        PTEXT_HIP(hipStreamSynchronize(st));
        PTEXT_HIP(hipGetLastError());
        const u64 total = last[0] + last[1];
        if (total > (u64)n * (u64)PTEXT_G_MAX) return PTEXT_FAIL(DSA_E_DEVICE, "internal: %llu text bytes of %lld values", total, (long long)n);
        *out_len = (int64_t)total;
        if ((int64_t)total > cap) return PTEXT_FAIL(DSA_E_CAPACITY, "the texts have %llu bytes", total);
        PTEXT_HIP(dout.reserve((size_t)total));
        hipLaunchKernelGGL(k_ptext_g_write, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const double*)dx.p, n, (const u64*)doff.p, dout.p, (int64_t)total);
        if (total) PTEXT_HIP(hipMemcpyAsync(out, dout.p, (size_t)total, hipMemcpyDeviceToHost, st));
        PTEXT_HIP(hipMemcpyAsync(len, dlen32.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PTEXT_HIP(hipStreamSynchronize(st));
        PTEXT_HIP(hipGetLastError());
        return DSA_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);                           // nothing is in flight when the buffers go
    return rc;
}

}  // extern "C"
