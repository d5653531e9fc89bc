// text_api.hip — the text front of the split-read chain on gfx950 (include/defuse_text.h): the improper-mate SAM text becomes
// cand_alignment[] (ParseSamLine, tools_src/defuse_host.hpp) and the FASTQ text a read store of bytes + bat_read[]
// (FastqReader::next + AddReads), both in device memory.
//
// Tables (both formats): the newline and tab positions of txt_shared.hpp, built by its host path like every other text's.
// SAM: one lane per line reads its tab positions 1-4 and 9-10 from the table and only qname, flag, rname and pos from the
//   text; the name is a binary search over the sorted names.  The first stop is an atomic minimum over the (rare) bad lines,
//   the carried read end an inclusive scan with "the last value told", the records are compacted by an exclusive sum of
//   their flags; everything at or behind the stop is cut off where those prefix results are read.
// FASTQ: one lane per group of four lines; two exclusive sums (packed kept / skipped counts, 64-bit sequence lengths) give
//   every kept record its slot and its offset, bat_shared.hpp's segmented gather copies the sequences behind those of the
//   earlier pieces.
// Every read of the text is at an index below len, or inside the zeroed padding of whole chunks behind it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/defuse_text.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "txt_names.hpp"
#include "txt_shared.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using hiphost::Keep;
using batdev::Seg64;

thread_local std::string g_txt_err;

#define TXT_HIP(call) HIPHOST_TRY(g_txt_err, call)
#define TXT_FAIL(code, ...) hiphost::fail(g_txt_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int READ_GROUP = 16;                // lanes per sequence in the gather, as bat_api.hip
constexpr uint8_t UNTOLD = 2;
static_assert(TEXT_PAD >= batdev::SRC_PAD + CHUNK, "padding");        // k_bat_gather reads the text

// ---- SAM --------------------------------------------------------------------------------------------------------------

// One lane per line.  kind 0 = a record (flag 1), 1 = skipped, 2.. = a stop; told = the read end the line tells, UNTOLD if it
// is carried or the line is no record.
__global__ __launch_bounds__(BLOCK) void k_sam_lines(Lines L, int64_t n_lines, NamesView nv, cand_alignment* __restrict__ al, uint8_t* __restrict__ told,
                                                     uint32_t* __restrict__ flag, uint32_t* __restrict__ stop)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_lines) return;
    const uint8_t* __restrict__ text = L.text;
    const int64_t s = line_start(L, i), e = line_end(L, i);
    const int64_t t0 = first_tab_rank(L, i), t1 = end_tab_rank(L, i);
    int kind = 0;
    uint8_t re = UNTOLD;
    cand_alignment a{-1, 0, 0, 0, -1, 0};
    if (e <= s) kind = TXT_SAM_EMPTY_LINE;
    else if (text[s] == '@') kind = 1;
    else if (t1 - t0 < 9 || t0 < 0 || t1 > L.n_tab) kind = TXT_SAM_FEW_FIELDS;
    else {
        const uint32_t* __restrict__ tp = L.tab_pos + t0;
        const int64_t q1 = tp[0], f1 = tp[1], r1 = tp[2], p1 = tp[3], s0 = tp[8];
        const int64_t s1 = t1 - t0 >= 10 ? (int64_t)tp[9] : e;
        int flg = 0, pos = 0;
        if (!field_int(text + q1 + 1, f1 - q1 - 1, flg) || !field_int(text + r1 + 1, p1 - r1 - 1, pos)) kind = TXT_SAM_BAD_INTEGER;
        else if (r1 - f1 - 1 == 1 && text[f1 + 1] == '*') kind = 1;
        else {
            int64_t slash = -1;
            int n_slash = 0;
            for (int64_t p = s; p < q1; ++p)
                if (text[p] == '/') {
                    if (n_slash == 0) slash = p;
                    ++n_slash;
                }
            int64_t frag_end = q1;
            if (n_slash == 1) {
                if (q1 - slash - 1 != 1 || (text[slash + 1] != '1' && text[slash + 1] != '2')) kind = TXT_SAM_BAD_QNAME;
                else {
                    frag_end = slash;
                    re = text[slash + 1] == '1' ? 0 : 1;
                }
            } else if (flg & 0x40) re = 0;
            else if (flg & 0x80) re = 1;
            if (kind == 0) {
                a.ref = find_name(nv, text + f1 + 1, r1 - f1 - 1);
                a.strand = (flg & 0x10) ? 1 : 0;
                a.start = pos;
                a.end = (int32_t)(uint32_t)(u64)((int64_t)pos + (s1 - s0 - 1) - 1);
                int frag = 0;
                a.fragment = (field_int(text + s, frag_end - s, frag) && frag >= 0) ? frag : -1;
                a.read_end = re;
            }
        }
    }
    if (kind >= 2) {
        atomicMin(stop, (uint32_t)i);
        a.ref = -kind;                             // (k_sam_result reads the stopping line's kind from here: no record, so ref is free)
    }
    al[i] = a;
    told[i] = kind == 0 ? re : UNTOLD;
    flag[i] = kind == 0 ? 1u : 0u;
}

struct LastTold {
    __host__ __device__ uint8_t operator()(uint8_t a, uint8_t b) const { return b != UNTOLD ? b : a; }
};

struct SamOut {
    int64_t consumed, n_lines, n_alignments, stop_line;
    u64 n_bad_fragment;
    int32_t stop_kind, carry_out;
    uint32_t stop;              // in: NONE; the lowest stopping line
    uint32_t pad_;
};

__global__ void k_sam_emit(const cand_alignment* __restrict__ al_line, const uint8_t* __restrict__ told_scan, const uint32_t* __restrict__ flag,
                           const uint32_t* __restrict__ pos, int64_t n_lines, int32_t carry_in, cand_alignment* __restrict__ out,
                           int32_t* __restrict__ line_of, SamOut* __restrict__ res)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_lines || (uint32_t)i >= res->stop || !flag[i] || (int64_t)pos[i] >= n_lines) return;
    cand_alignment a = al_line[i];
    a.read_end = told_scan[i] != UNTOLD ? (int32_t)told_scan[i] : carry_in;
    out[pos[i]] = a;
    line_of[pos[i]] = (int32_t)(i + 1);
    if (a.fragment < 0) atomicAdd(&res->n_bad_fragment, 1ull);
}

// one thread, after k_sam_emit (which reads res->stop and adds to n_bad_fragment)
__global__ void k_sam_result(Lines L, int64_t n_lines, const cand_alignment* __restrict__ al_line, const uint8_t* __restrict__ told_scan,
                             const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, int32_t carry_in, SamOut* __restrict__ res)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool stopped = (int64_t)res->stop < n_lines;
    const int64_t c = stopped ? (int64_t)res->stop : n_lines;          // lines consumed
    res->n_lines = c;
    res->n_alignments = c ? (int64_t)pos[c - 1] + (int64_t)flag[c - 1] : 0;
    res->carry_out = (c && told_scan[c - 1] != UNTOLD) ? (int32_t)told_scan[c - 1] : carry_in;
    res->consumed = c == 0 ? 0 : (c - 1 < L.n_nl ? (int64_t)L.nl_pos[c - 1] + 1 : L.len);
    res->stop_line = stopped ? c + 1 : 0;
    res->stop_kind = stopped ? -al_line[c].ref : 0;
}

// ---- FASTQ ------------------------------------------------------------------------------------------------------------

struct FqRec {
    int64_t seq;                // where the sequence begins in the text
    int32_t len, fragment, read_end;
    int32_t kind;               // 0 kept, -1 skipped, 1.. a stop
};

__global__ __launch_bounds__(BLOCK) void k_fq_records(Lines L, int64_t n_rec, int32_t max_len, FqRec* __restrict__ rec, u64* __restrict__ cnt,
                                                      u64* __restrict__ slen, uint32_t* __restrict__ stop)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_rec) return;
    const uint8_t* __restrict__ text = L.text;
    const int64_t s = line_start(L, 4 * g), e = line_end(L, 4 * g);
    const int64_t q0 = line_start(L, 4 * g + 1), q1 = line_end(L, 4 * g + 1);
    FqRec r{q0, 0, 0, 0, 0};
    if (e <= s || text[s] != '@') r.kind = TXT_FASTQ_BAD_NAME;
    else {
        int64_t slash = s + 1;
        while (slash < e && text[slash] != '/') ++slash;
        const uint8_t endc = slash + 1 < e ? text[slash + 1] : 0;
        if (endc != '1' && endc != '2') r.kind = TXT_FASTQ_BAD_END;
        else if (!field_int(text + s + 1, slash - s - 1, r.fragment)) r.kind = TXT_FASTQ_BAD_FRAGMENT;
        else if (q1 - q0 >= (int64_t)max_len) r.kind = TXT_FASTQ_LONG_READ;
        else {
            r.read_end = endc == '1' ? 0 : 1;
            r.len = (int32_t)(q1 - q0);
            if (r.fragment < 0) r.kind = -1;
        }
    }
    if (r.kind > 0) atomicMin(stop, (uint32_t)g);
    rec[g] = r;
    cnt[g] = r.kind == 0 ? 1ull : r.kind < 0 ? (1ull << 32) : 0ull;           // kept in the low word, skipped in the high word
    slen[g] = r.kind == 0 ? (u64)r.len : 0ull;
}

struct FqOut {
    int64_t n_groups;           // groups consumed (in front of the stop)
    int64_t n_records, n_skipped, n_bytes;
    int64_t consumed;           // the end of the last of these groups' lines
    int32_t stop_kind;
    uint32_t stop;              // in: NONE
};

__global__ void k_fq_result(Lines L, int64_t n_rec, const FqRec* __restrict__ rec, const u64* __restrict__ cnt, const u64* __restrict__ cpos,
                            const u64* __restrict__ slen, const u64* __restrict__ soff, FqOut* __restrict__ res)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool stopped = (int64_t)res->stop < n_rec;
    const int64_t c = stopped ? (int64_t)res->stop : n_rec;
    const u64 counts = c ? cpos[c - 1] + cnt[c - 1] : 0;
    res->n_groups = c;
    res->n_records = (int64_t)(counts & 0xFFFFFFFFull);
    res->n_skipped = (int64_t)(counts >> 32);
    res->n_bytes = c ? (int64_t)(soff[c - 1] + slen[c - 1]) : 0;
    res->consumed = c == 0 ? 0 : (4 * c - 1 < L.n_nl ? (int64_t)L.nl_pos[4 * c - 1] + 1 : L.len);
    res->stop_kind = stopped ? rec[c].kind : 0;
}

__global__ void k_fq_emit(const FqRec* __restrict__ rec, const u64* __restrict__ cpos, const u64* __restrict__ soff, int64_t n_groups, int64_t n_records,
                          int64_t reads_before, int64_t bytes_before, bat_read* __restrict__ reads, Seg64* __restrict__ seg)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    const FqRec r = rec[g];
    const int64_t p = (int64_t)(cpos[g] & 0xFFFFFFFFull);
    if (r.kind != 0 || p >= n_records) return;
    const int64_t off = bytes_before + (int64_t)soff[g];
    reads[reads_before + p] = bat_read{off, r.len, r.fragment, r.read_end, 0};
    seg[p] = Seg64{r.seq, off, (uint32_t)r.len, 0u};
}

}  // namespace

struct txt_names : NameTable {};

struct txt_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[5];        // 0 start, 1 text on the device, 2 kernels done; 3, 4 around a fetch
    txt_timing timing{};
    int32_t max_read_len = TXT_MAX_READ_LEN;
    // the text and its tables
    DeviceBuffer<uint8_t, GrowSize> text;
    TextScratch scratch;
    TextTables tables;
    Totals tot{};
    // SAM
    DeviceBuffer<cand_alignment, GrowSize> al_line, al;
    DeviceBuffer<uint8_t, GrowSize> told, told_scan;
    DeviceBuffer<uint32_t, GrowSize> flag, pos;
    DeviceBuffer<int32_t, GrowSize> line_of;
    DeviceBuffer<SamOut> sam_out;
    int64_t n_al = 0;
    // FASTQ
    DeviceBuffer<FqRec, GrowSize> fq_rec;
    DeviceBuffer<u64, GrowSize> cnt, cpos, slen, soff;
    DeviceBuffer<Seg64, GrowSize> seg;
    DeviceBuffer<FqOut> fq_out;
    DeviceBuffer<uint8_t, GrowSize> store_bytes;
    DeviceBuffer<bat_read, GrowSize> store_reads;
    int64_t store_bytes_len = 0, store_n = 0;
    int64_t file_lines = 0;      // lines of the current file consumed by earlier pieces
    int32_t file_stop_kind = 0;
    int64_t file_stop_line = 0;
};

namespace {

// The text into the ctx (padded with zeros) and its tables.  `len` > 0.  On return c->tot holds the totals and the tables
// are being written; the stream has been synchronised once (for the totals).
template <bool TABS>
int build_tables(txt_ctx* c, const void* text, int64_t len, bool on_device, Lines* L)
{
    TXT_HIP(c->text.reserve(padded_size(len)));
    if (const int rc = text_upload_count<TABS>(g_txt_err, c->scratch, c->text.p, text, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, len, c->ev[0],
                                               c->ev[1], c->st, c->tot))
        return rc;
    TXT_HIP(c->tables.reserve(c->tot));
    *L = c->tables.place<TABS>(c->scratch, c->text.p, len, c->tot, c->st);
    return DSA_OK;
}

int parse_sam_run(txt_ctx* c, const txt_names* names, const void* text, int64_t len, int32_t final, int32_t carry_in, txt_sam_result* result, bool on_device);

int parse_sam(const char* what, txt_ctx* c, const txt_names* names, const void* text, int64_t len, int32_t final, int32_t carry_in, txt_sam_result* result,
              bool on_device)
{
    if (!result) return TXT_FAIL(DSA_E_ARG, "%s: no result", what);
    *result = txt_sam_result{0, 0, 0, 0, 0, 0, carry_in};
    if (len < 0) return TXT_FAIL(DSA_E_ARG, "%s: negative length (%lld)", what, (long long)len);
    if (len > (int64_t)INT32_MAX) return TXT_FAIL(DSA_E_LIMIT, "%s: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", what, (long long)len);
    if (len && !text) return TXT_FAIL(DSA_E_ARG, "%s: null pointer with non-zero size", what);
    if (final != 0 && final != 1) return TXT_FAIL(DSA_E_ARG, "%s: final %d is not 0 or 1", what, final);
    if (carry_in != 0 && carry_in != 1) return TXT_FAIL(DSA_E_ARG, "%s: carry_in %d is not 0 or 1", what, carry_in);
    if (!c || !names) return TXT_FAIL(DSA_E_ARG, "%s: no %s", what, !c ? "ctx" : "names");
    if (c->device != names->device) return TXT_FAIL(DSA_E_ARG, "%s: ctx and names are on devices %d and %d", what, c->device, names->device);
    c->n_al = 0;
    c->timing = txt_timing{0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = parse_sam_run(c, names, text, len, final, carry_in, result, on_device);
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);          // nothing of a refused call is in flight when it returns
    return rc;
}

int parse_sam_run(txt_ctx* c, const txt_names* names, const void* text, int64_t len, int32_t final, int32_t carry_in, txt_sam_result* result, bool on_device)
{
    TXT_HIP(hipSetDevice(c->device));
    TXT_HIP(c->al.reserve(1));                      // the view of an empty result has pointers too
    TXT_HIP(c->line_of.reserve(1));
    if (!on_device && !final) len = whole_lines(static_cast<const uint8_t*>(text), len);
    if (len == 0) return DSA_OK;
    hipStream_t st = c->st;
    Lines L{};
    if (const int rc = build_tables<true>(c, text, len, on_device, &L)) return rc;
    const int64_t n_lines = (int64_t)c->tot.n_nl + ((final && c->tot.last != '\n') ? 1 : 0);
    c->timing.text_bytes = len;
    if (n_lines == 0) {                             // (a device text without a newline and final = 0)
        TXT_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    }
    TXT_HIP(c->al_line.reserve((size_t)n_lines));
    TXT_HIP(c->al.reserve((size_t)n_lines));
    TXT_HIP(c->line_of.reserve((size_t)n_lines));
    TXT_HIP(c->told.reserve((size_t)n_lines));
    TXT_HIP(c->told_scan.reserve((size_t)n_lines));
    TXT_HIP(c->flag.reserve((size_t)n_lines));
    TXT_HIP(c->pos.reserve((size_t)n_lines));
    TXT_HIP(c->sam_out.reserve(1));
    SamOut out{};
    out.stop = NONE;
    TXT_HIP(hipMemcpyAsync(c->sam_out.p, &out, sizeof(SamOut), hipMemcpyHostToDevice, st));
    const unsigned gl = grid_of(n_lines);
    hipLaunchKernelGGL(k_sam_lines, dim3(gl), dim3(BLOCK), 0, st, L, n_lines, names->view(), c->al_line.p, c->told.p, c->flag.p, &c->sam_out.p->stop);
    TXT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceScan::InclusiveScan(w, wb, c->told.p, c->told_scan.p, LastTold(), (int)n_lines, st);
    }));
    TXT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->flag.p, c->pos.p, (int)n_lines, st); }));
    hipLaunchKernelGGL(k_sam_emit, dim3(gl), dim3(BLOCK), 0, st, (const cand_alignment*)c->al_line.p, (const uint8_t*)c->told_scan.p, (const uint32_t*)c->flag.p,
                       (const uint32_t*)c->pos.p, n_lines, carry_in, c->al.p, c->line_of.p, c->sam_out.p);
    hipLaunchKernelGGL(k_sam_result, dim3(1), dim3(64), 0, st, L, n_lines, (const cand_alignment*)c->al_line.p, (const uint8_t*)c->told_scan.p,
                       (const uint32_t*)c->flag.p, (const uint32_t*)c->pos.p, carry_in, c->sam_out.p);
    TXT_HIP(hipEventRecord(c->ev[2], st));
    TXT_HIP(hipMemcpyAsync(&out, c->sam_out.p, sizeof(SamOut), hipMemcpyDeviceToHost, st));
    TXT_HIP(hipStreamSynchronize(st));
    TXT_HIP(hipGetLastError());
    if (out.n_alignments < 0 || out.n_alignments > out.n_lines || out.n_lines > n_lines || out.consumed < 0 || out.consumed > len)
        return TXT_FAIL(DSA_E_DEVICE, "internal: %lld alignments of %lld lines", (long long)out.n_alignments, (long long)out.n_lines);
    *result = txt_sam_result{out.consumed, out.n_lines, out.n_alignments, out.stop_line, (int64_t)out.n_bad_fragment, out.stop_kind, out.carry_out};
    c->n_al = out.n_alignments;
    c->timing.upload_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.device_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.n_lines = out.n_lines;
    c->timing.n_records = out.n_alignments;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* txt_last_error(void) { return g_txt_err.c_str(); }

int txt_names_create(int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off, int64_t n_names, txt_names** out)
{
    if (!out) return TXT_FAIL(DSA_E_ARG, "txt_names_create: no output");
    *out = nullptr;
    txt_names* nm = new txt_names();
    if (const int rc = name_table_create(g_txt_err, "txt_names_create", device, name_bytes, name_bytes_len, name_off, n_names, nm)) {
        delete nm;
        return rc;
    }
    *out = nm;
    return DSA_OK;
}

void txt_names_destroy(txt_names* names)
{
    if (!names) return;
    (void)hipSetDevice(names->device);
    delete names;
}

int txt_create(int device, txt_ctx** out)
{
    if (!out) return TXT_FAIL(DSA_E_ARG, "txt_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_txt_err)) return DSA_E_DEVICE;
    TXT_HIP(hipSetDevice(device));
    txt_ctx* c = new txt_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    ok = ok && c->al.reserve(1) == hipSuccess && c->line_of.reserve(1) == hipSuccess && c->store_bytes.reserve(4) == hipSuccess &&
         c->store_reads.reserve(1) == hipSuccess;
    if (!ok) {
        delete c;
        return TXT_FAIL(DSA_E_DEVICE, "cannot create a stream or a buffer");
    }
    *out = c;
    return DSA_OK;
}

void txt_destroy(txt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int txt_set_max_read_len(txt_ctx* c, int32_t max_read_len)
{
    if (!c) return TXT_FAIL(DSA_E_ARG, "txt_set_max_read_len: no ctx");
    if (max_read_len < 1 || max_read_len > TXT_MAX_READ_LEN) return TXT_FAIL(DSA_E_ARG, "max_read_len %d is outside [1, %d]", max_read_len, TXT_MAX_READ_LEN);
    c->max_read_len = max_read_len;
    return DSA_OK;
}

int txt_parse_sam(txt_ctx* c, const txt_names* names, const uint8_t* text, int64_t len, int32_t final, int32_t carry_in, txt_sam_result* result)
{
    return parse_sam("txt_parse_sam", c, names, text, len, final, carry_in, result, false);
}

int txt_parse_sam_device(txt_ctx* c, const txt_names* names, const void* text_device, int64_t len, int32_t final, int32_t carry_in, txt_sam_result* result)
{
    return parse_sam("txt_parse_sam_device", c, names, text_device, len, final, carry_in, result, true);
}

int txt_sam_view(const txt_ctx* c, txt_sam_device_view* out)
{
    if (!c || !out) return TXT_FAIL(DSA_E_ARG, "txt_sam_view: no %s", !c ? "ctx" : "output");
    *out = txt_sam_device_view{c->al.p, c->line_of.p, c->n_al, c->device, 0};
    return DSA_OK;
}

int txt_sam_fetch(txt_ctx* c, cand_alignment* alignments, int64_t cap, int32_t* line_of, int64_t line_cap)
{
    if (!c) return TXT_FAIL(DSA_E_ARG, "txt_sam_fetch: no ctx");
    if (cap < 0 || line_cap < 0) return TXT_FAIL(DSA_E_ARG, "txt_sam_fetch: negative capacity");
    if ((cap && !alignments) || (line_cap && !line_of)) return TXT_FAIL(DSA_E_ARG, "txt_sam_fetch: capacity without a buffer");
    if (cap < c->n_al || (line_cap && line_cap < c->n_al)) return TXT_FAIL(DSA_E_CAPACITY, "the parse has %lld alignments", (long long)c->n_al);
    TXT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    TXT_HIP(hipEventRecord(c->ev[3], st));
    if (c->n_al) TXT_HIP(hipMemcpyAsync(alignments, c->al.p, (size_t)c->n_al * sizeof(cand_alignment), hipMemcpyDeviceToHost, st));
    if (c->n_al && line_cap) TXT_HIP(hipMemcpyAsync(line_of, c->line_of.p, (size_t)c->n_al * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TXT_HIP(hipEventRecord(c->ev[4], st));
    TXT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    return DSA_OK;
}

int txt_fastq_begin(txt_ctx* c)
{
    if (!c) return TXT_FAIL(DSA_E_ARG, "txt_fastq_begin: no ctx");
    c->store_bytes_len = c->store_n = 0;
    c->file_lines = c->file_stop_line = 0;
    c->file_stop_kind = 0;
    return DSA_OK;
}

int txt_fastq_add(txt_ctx* c, const uint8_t* text, int64_t len, int32_t final, txt_fastq_result* result)
{
    if (!result) return TXT_FAIL(DSA_E_ARG, "txt_fastq_add: no result");
    *result = txt_fastq_result{0, 0, 0, 0, 0, 0};
    if (len < 0) return TXT_FAIL(DSA_E_ARG, "txt_fastq_add: negative length (%lld)", (long long)len);
    if (len > (int64_t)INT32_MAX) return TXT_FAIL(DSA_E_LIMIT, "txt_fastq_add: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", (long long)len);
    if (len && !text) return TXT_FAIL(DSA_E_ARG, "txt_fastq_add: null pointer with non-zero size");
    if (final != 0 && final != 1) return TXT_FAIL(DSA_E_ARG, "txt_fastq_add: final %d is not 0 or 1", final);
    if (!c) return TXT_FAIL(DSA_E_ARG, "txt_fastq_add: no ctx");
    c->timing = txt_timing{0, 0, 0, 0, 0, 0, 0, 0};
    auto end_of_file = [&]() {
        if (final) {
            c->file_lines = c->file_stop_line = 0;
            c->file_stop_kind = 0;
        }
    };
    if (c->file_stop_kind) {                        // the file has ended at its stop: its further pieces are passed over
        *result = txt_fastq_result{len, 0, 0, c->file_stop_line, c->file_stop_kind, 0};
        end_of_file();
        return DSA_OK;
    }
    const int64_t given = len;
    if (!final) len = whole_lines(text, len);
    if (len == 0) {
        end_of_file();
        return DSA_OK;
    }
    auto run = [&]() -> int {
        TXT_HIP(hipSetDevice(c->device));
        hipStream_t st = c->st;
        Lines L{};
        if (const int rc = build_tables<false>(c, text, len, false, &L)) return rc;
        c->timing.text_bytes = len;
        const int64_t n_lines = (int64_t)c->tot.n_nl + ((final && c->tot.last != '\n') ? 1 : 0);
        const int64_t n_rec = n_lines / 4;
        if (n_rec == 0) {
            TXT_HIP(hipStreamSynchronize(st));
            result->consumed = final ? given : 0;
            return DSA_OK;
        }
        TXT_HIP(c->fq_rec.reserve((size_t)n_rec));
        TXT_HIP(c->cnt.reserve((size_t)n_rec));
        TXT_HIP(c->cpos.reserve((size_t)n_rec));
        TXT_HIP(c->slen.reserve((size_t)n_rec));
        TXT_HIP(c->soff.reserve((size_t)n_rec));
        TXT_HIP(c->fq_out.reserve(1));
        FqOut out{};
        out.stop = NONE;
        TXT_HIP(hipMemcpyAsync(c->fq_out.p, &out, sizeof(FqOut), hipMemcpyHostToDevice, st));
        const unsigned gr = grid_of(n_rec);
        hipLaunchKernelGGL(k_fq_records, dim3(gr), dim3(BLOCK), 0, st, L, n_rec, c->max_read_len, c->fq_rec.p, c->cnt.p, c->slen.p, &c->fq_out.p->stop);
        TXT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->cnt.p, c->cpos.p, (int)n_rec, st); }));
        TXT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->slen.p, c->soff.p, (int)n_rec, st); }));
        hipLaunchKernelGGL(k_fq_result, dim3(1), dim3(64), 0, st, L, n_rec, (const FqRec*)c->fq_rec.p, (const u64*)c->cnt.p, (const u64*)c->cpos.p,
                           (const u64*)c->slen.p, (const u64*)c->soff.p, c->fq_out.p);
        TXT_HIP(hipMemcpyAsync(&out, c->fq_out.p, sizeof(FqOut), hipMemcpyDeviceToHost, st));
        TXT_HIP(hipStreamSynchronize(st));
        TXT_HIP(hipGetLastError());
        if (out.n_groups < 0 || out.n_groups > n_rec || out.n_records < 0 || out.n_records + out.n_skipped > out.n_groups || out.n_bytes < 0 || out.n_bytes > len)
            return TXT_FAIL(DSA_E_DEVICE, "internal: %lld records of %lld groups, %lld bytes", (long long)out.n_records, (long long)out.n_groups, (long long)out.n_bytes);
        if (out.n_records) {
            TXT_HIP(hiphost::grow_keep(c->store_reads, Keep{(size_t)c->store_n}, (size_t)(c->store_n + out.n_records), st));
            TXT_HIP(hiphost::grow_keep(c->store_bytes, Keep{(size_t)c->store_bytes_len}, (size_t)(c->store_bytes_len + out.n_bytes) + 4, st));            // whole dwords
            TXT_HIP(c->seg.reserve((size_t)out.n_records));
            hipLaunchKernelGGL(k_fq_emit, dim3(grid_of(out.n_groups)), dim3(BLOCK), 0, st, (const FqRec*)c->fq_rec.p, (const u64*)c->cpos.p, (const u64*)c->soff.p,
                               out.n_groups, out.n_records, c->store_n, c->store_bytes_len, c->store_reads.p, c->seg.p);
            hipLaunchKernelGGL((k_bat_gather<READ_GROUP, false, Seg64>), dim3(grid_of(out.n_records * READ_GROUP)), dim3(BLOCK), 0, st, (const Seg64*)c->seg.p,
                               out.n_records, (const uint8_t*)c->text.p, len, c->store_bytes.p, c->store_bytes_len + out.n_bytes);
        }
        TXT_HIP(hipEventRecord(c->ev[2], st));
        TXT_HIP(hipStreamSynchronize(st));
        TXT_HIP(hipGetLastError());
        c->store_n += out.n_records;
        c->store_bytes_len += out.n_bytes;
        result->n_records = out.n_records;
        result->n_skipped = out.n_skipped;
        if (out.stop_kind) {
            result->stop_kind = c->file_stop_kind = out.stop_kind;
            result->stop_line = c->file_stop_line = c->file_lines + 4 * out.n_groups + 1;
            result->consumed = given;
        } else {
            result->consumed = final ? given : out.consumed;
            c->file_lines += 4 * out.n_groups;
        }
        c->timing.upload_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
        c->timing.device_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
        c->timing.n_lines = 4 * out.n_groups;
        c->timing.n_records = out.n_records;
        c->timing.gather_bytes = out.n_bytes;
        return DSA_OK;
    };
    const int rc = run();
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);
    else end_of_file();
    return rc;
}

int txt_fastq_view(const txt_ctx* c, txt_fastq_device_view* out)
{
    if (!c || !out) return TXT_FAIL(DSA_E_ARG, "txt_fastq_view: no %s", !c ? "ctx" : "output");
    *out = txt_fastq_device_view{c->store_bytes.p, c->store_reads.p, c->store_bytes_len, c->store_n, c->device, 0};
    return DSA_OK;
}

int txt_fastq_fetch(txt_ctx* c, uint8_t* bytes, int64_t bytes_cap, bat_read* reads, int64_t reads_cap)
{
    if (!c) return TXT_FAIL(DSA_E_ARG, "txt_fastq_fetch: no ctx");
    if (bytes_cap < 0 || reads_cap < 0) return TXT_FAIL(DSA_E_ARG, "txt_fastq_fetch: negative capacity");
    if ((bytes_cap && !bytes) || (reads_cap && !reads)) return TXT_FAIL(DSA_E_ARG, "txt_fastq_fetch: capacity without a buffer");
    if (bytes_cap < c->store_bytes_len || reads_cap < c->store_n)
        return TXT_FAIL(DSA_E_CAPACITY, "the store has %lld bytes and %lld reads", (long long)c->store_bytes_len, (long long)c->store_n);
    TXT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    TXT_HIP(hipEventRecord(c->ev[3], st));
    if (c->store_bytes_len) TXT_HIP(hipMemcpyAsync(bytes, c->store_bytes.p, (size_t)c->store_bytes_len, hipMemcpyDeviceToHost, st));
    if (c->store_n) TXT_HIP(hipMemcpyAsync(reads, c->store_reads.p, (size_t)c->store_n * sizeof(bat_read), hipMemcpyDeviceToHost, st));
    TXT_HIP(hipEventRecord(c->ev[4], st));
    TXT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    return DSA_OK;
}

int txt_get_timing(const txt_ctx* c, txt_timing* out)
{
    if (!c || !out) return TXT_FAIL(DSA_E_ARG, "txt_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
