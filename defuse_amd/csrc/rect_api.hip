// rect_api.hip — the way into the record store for an alignment FILE on gfx950 (include/defuse_rec.h, section "alignment
// text"): one piece of splitreads.alignments goes up as text, and the records of its lines are written straight behind the
// store's last record (rec_tail / rec_commit), so that rec_sort and rec_text can bring the sorted file down.
//
// A piece (rect_add), n_lines lines:
//   tables  the newline and tab positions of txt_shared.hpp, tabs included;
//   parse   k_rect_lines: lane i takes line i, finds its fields in the tab table, applies rect_shared.hpp's rule and writes the
//           40-byte record at tail index i.  Every line in front of the stop gives exactly one record, so the record index is
//           the line index and nothing is compacted; records written behind the stop are not committed.  The stop is an
//           atomic minimum over the (rare) stopping lines; the lines that are not plain are counted, and the lowest of them
//           found, by one block reduction each and one atomic per workgroup that has any;
//   result  the host reads the stop.  If there is one, k_rect_lines<false> counts the lines that are not plain among those in
//           front of it (no stores); k_rect_result re-reads the stopping line for its kind, field and id.
// Every read of the text is below its length or inside the zeroed padding of whole chunks behind it; every table is indexed
// below its count; every record store is at an index below n_lines, the room rec_tail gave.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <string>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_rec.h"
#include "hip_host.hpp"
#include "rect_shared.hpp"
#include "txt_shared.hpp"

__attribute__((visibility("hidden"))) int recstore_device(const rec_store* s);      // rec_api.hip

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;

thread_local std::string g_rect_err;

#define RECT_HIP(call) HIPHOST_TRY(g_rect_err, call)
#define RECT_FAIL(code, ...) hiphost::fail(g_rect_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;

static_assert(sizeof(dsa_record) == 40 && sizeof(rect_result) == 64 && sizeof(rect_timing) == 32, "C ABI layout");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct RectOut {
    rect_result r;
    uint32_t stop;              // in: NONE; the lowest stopping line
    uint32_t other;             // in: NONE; the lowest line that is not plain
    u64 others;                 // lines that are not plain, over all lines
    u64 others_before;          // the same over the lines in front of the stop (counted only if there is one)
};

// line i < n_lines of the text
__device__ inline rect_line parse_at(const Lines& L, int64_t i)
{
    const LineAt a = line_at(L, i);
    return rect_parse_line(L.text, a.s, a.e, a.n_tabs, TabAt{L.tab_pos + a.t0}, DeviceInt());
}

// A record is ten ints at a multiple of 40 bytes from an allocation's start: 8-byte aligned (rec_load of rec_api.hip).
__device__ inline void rec_put(dsa_record* p, const dsa_record& r)
{
    char* b = static_cast<char*>(__builtin_assume_aligned(p, 8));
    const u32x4 lo = {(uint32_t)r.fusion_id, (uint32_t)r.frag, (uint32_t)r.read_end, (uint32_t)r.revcomp};
    const u32x4 mid = {(uint32_t)r.ref_first, (uint32_t)r.ref_second, (uint32_t)r.read_first, (uint32_t)r.read_second};
    const u32x2 hi = {(uint32_t)r.score, (uint32_t)r.pair_idx};
    __builtin_memcpy(b, &lo, 16);
    __builtin_memcpy(b + 16, &mid, 16);
    __builtin_memcpy(b + 32, &hi, 8);
}

// One lane per line.  WRITE: the record to tail[i], the stop and the lowest line that is not plain; without it only the count
// of such lines (into others_before), for the lines in front of a stop.
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void k_rect_lines(Lines L, int64_t n_lines, dsa_record* __restrict__ tail, RectOut* __restrict__ res)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp[2];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t other = 0, first = NONE;
    if (i < n_lines) {
        const rect_line r = parse_at(L, i);
        if (r.kind) {
            if (WRITE) atomicMin(&res->stop, (uint32_t)i);
        } else {
            if (WRITE) rec_put(tail + i, r.rec);
            if (!r.plain) {
                other = 1;
                first = (uint32_t)i;
            }
        }
    }
    const uint32_t n = Reduce(tmp[0]).Sum(other);                  // (every lane of the workgroup is here)
    const uint32_t lowest = Reduce(tmp[1]).Reduce(first, hipcub::Min());
    if (threadIdx.x == 0 && n) {
        atomicAdd(WRITE ? &res->others : &res->others_before, (u64)n);
        if (WRITE) atomicMin(&res->other, lowest);
    }
}

// one thread, after the line kernels
__global__ void k_rect_result(Lines L, int64_t n_lines, RectOut* __restrict__ res)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool stopped = (int64_t)res->stop < n_lines;
    const int64_t c = stopped ? (int64_t)res->stop : n_lines;     // lines consumed
    rect_result r{};
    r.n_lines = r.n_records = c;
    r.consumed = c == 0 ? 0 : (c - 1 < L.n_nl ? (int64_t)L.nl_pos[c - 1] + 1 : L.len);
    r.stop_field = -1;
    if (stopped) {
        const rect_line s = parse_at(L, c);
        r.stop_line = c + 1;
        r.stop_kind = s.kind;
        r.stop_field = s.field;
        r.stop_id_read = s.id_read;
        r.stop_id = s.id;
    }
    r.n_other = (int64_t)(stopped ? res->others_before : res->others);
    r.first_other = (int64_t)res->other < c ? (int64_t)res->other + 1 : 0;
    res->r = r;
}

}  // namespace

struct rect_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[3];
    rect_timing timing{};
    DeviceBuffer<uint8_t, GrowSize> text;
    TextScratch scratch;
    TextTables tables;
    DeviceBuffer<RectOut> out;
};

namespace {

// `len` > 0
int add_run(rect_ctx* c, rec_store* store, const uint8_t* text, int64_t len, int32_t final, rect_result* result)
{
    RECT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    RECT_HIP(c->text.reserve(padded_size(len)));
    RECT_HIP(c->out.reserve(1));
    Totals tot{};
    if (const int rc = text_upload_count<true>(g_rect_err, c->scratch, c->text.p, text, hipMemcpyHostToDevice, len, c->ev[0], c->ev[1], st, tot)) return rc;
    const int64_t n_lines = (int64_t)tot.n_nl + ((final && tot.last != '\n') ? 1 : 0);      // at least one: the text is not empty
    // room behind the store's last record, one record per line; the store's bound is checked here, before anything is written
    void* tail = nullptr;
    if (const int rc = rec_tail(store, n_lines, &tail)) return RECT_FAIL(rc, "rect_add: %s", rec_last_error());
    RECT_HIP(hipSetDevice(c->device));
    RECT_HIP(c->tables.reserve(tot));
    const Lines L = c->tables.place<true>(c->scratch, c->text.p, len, tot, st);
    RectOut out{};
    out.stop = out.other = NONE;
    RECT_HIP(hipMemcpyAsync(c->out.p, &out, sizeof(RectOut), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rect_lines<true>, dim3(grid_of(n_lines)), dim3(BLOCK), 0, st, L, n_lines, static_cast<dsa_record*>(tail), c->out.p);
    uint32_t stop = NONE;
    RECT_HIP(hipMemcpyAsync(&stop, &c->out.p->stop, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RECT_HIP(hipStreamSynchronize(st));
    RECT_HIP(hipGetLastError());
    if ((int64_t)stop < n_lines && stop > 0)
        hipLaunchKernelGGL(k_rect_lines<false>, dim3(grid_of((int64_t)stop)), dim3(BLOCK), 0, st, L, (int64_t)stop, (dsa_record*)nullptr, c->out.p);
    hipLaunchKernelGGL(k_rect_result, dim3(1), dim3(64), 0, st, L, n_lines, c->out.p);
    RECT_HIP(hipEventRecord(c->ev[2], st));
    RECT_HIP(hipMemcpyAsync(&out, c->out.p, sizeof(RectOut), hipMemcpyDeviceToHost, st));
    RECT_HIP(hipStreamSynchronize(st));
    RECT_HIP(hipGetLastError());
    const rect_result& r = out.r;
    if (r.n_records < 0 || r.n_records > n_lines || r.consumed < 0 || r.consumed > len || r.n_other < 0 || r.n_other > r.n_records)
        return RECT_FAIL(DSA_E_DEVICE, "internal: %lld records of %lld lines, %lld of %lld bytes", (long long)r.n_records, (long long)n_lines, (long long)r.consumed,
                         (long long)len);
    if (const int rc = rec_commit(store, r.n_records)) return RECT_FAIL(rc, "rect_add: %s", rec_last_error());
    *result = r;
    c->timing.upload_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.device_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.text_bytes = len;
    c->timing.n_lines = r.n_lines;
    c->timing.n_records = r.n_records;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* rect_last_error(void) { return g_rect_err.c_str(); }

int rect_create(int device, rect_ctx** out)
{
    if (!out) return RECT_FAIL(DSA_E_ARG, "rect_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_rect_err)) return DSA_E_DEVICE;
    RECT_HIP(hipSetDevice(device));
    rect_ctx* c = new rect_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return RECT_FAIL(DSA_E_DEVICE, "rect_create: cannot create a stream or an event");
    }
    *out = c;
    return DSA_OK;
}

void rect_destroy(rect_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int rect_add(rect_ctx* c, rec_store* store, const uint8_t* text, int64_t len, int32_t final, rect_result* result)
{
    if (!result) return RECT_FAIL(DSA_E_ARG, "rect_add: no result");
    *result = rect_result{};
    result->stop_field = -1;
    if (len < 0) return RECT_FAIL(DSA_E_ARG, "rect_add: negative length (%lld)", (long long)len);
    if (len > (int64_t)INT32_MAX) return RECT_FAIL(DSA_E_LIMIT, "rect_add: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", (long long)len);
    if (len && !text) return RECT_FAIL(DSA_E_ARG, "rect_add: null pointer with non-zero size");
    if (final != 0 && final != 1) return RECT_FAIL(DSA_E_ARG, "rect_add: final %d is not 0 or 1", final);
    if (!c || !store) return RECT_FAIL(DSA_E_ARG, "rect_add: no %s", !c ? "ctx" : "store");
    if (c->device != recstore_device(store)) return RECT_FAIL(DSA_E_ARG, "rect_add: ctx and store are on devices %d and %d", c->device, recstore_device(store));
    c->timing = rect_timing{};
    if (!final) len = whole_lines(text, len);
    if (len == 0) return DSA_OK;
    const int rc = add_run(c, store, text, len, final, result);
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);          // nothing of a refused call is in flight when it returns
    return rc;
}

int rect_get_timing(const rect_ctx* c, rect_timing* out)
{
    if (!c || !out) return RECT_FAIL(DSA_E_ARG, "rect_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
