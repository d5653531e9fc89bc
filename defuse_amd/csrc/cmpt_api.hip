// cmpt_api.hip — the text front and back of clustermatepairs on gfx950 (include/defuse_cmp.h, section "alignment and cluster
// text"): the compact alignment file goes up in pieces and becomes records, fragment starts and reference names in device
// memory; the rows of cmp_problems_select become the bytes of the cluster file there.
//
// A piece (cmpt_add) is copied into a buffer padded with zeros and gets the newline and tab tables of txt_shared.hpp.  Then
//   lines    k_cmpt_lines: one lane per line takes its fields from the tab table, writes the record (without its reference
//            index), the line's kind and whether its field 0 differs from that of the line before (the first line of a piece
//            compares with the bytes carried from the piece before); the first stop is an atomic minimum over the (rare)
//            stopping lines.  The host reads it: only the lines before it go on.
//   names    the dictionary is an open-addressing table over the stream.  A slot holds EMPTY, a name of an earlier piece
//            (KNOWN | index) or the line of this piece whose lane claimed it (compare-and-swap).  k_cmpt_probe: a lane hashes
//            its name and walks the slots from there; at every taken slot it compares BYTES, with the dictionary or with the
//            claiming line, and moves on only if they differ, so a hash never decides equality.  At its slot it lowers the
//            slot's first line by an atomic minimum, and only if a plain read says that it would: thousands of lines with one
//            name issue a handful of atomics.  k_cmpt_rank flags the line that is its slot's first; an exclusive sum over the
//            flags ranks the new names by first line, one over their lengths places their bytes; k_cmpt_assign appends them to
//            the dictionary behind the names of the earlier pieces and turns their slots into KNOWN ones.
//   layout   an exclusive sum over the fragment flags; k_cmpt_refs completes every record with its reference index and writes
//            the fragment starts; k_cmpt_close closes them with the number of records.
// The printer is a length pass (one lane per output line), one 64-bit exclusive sum and a write pass: a lane writes its whole
// line, so every output byte has one writer.
//
// Bounds: every read of a piece's text is below its length or inside the zeroed padding of whole chunks behind it; per-line
// arrays hold n_lines + 1 elements and are indexed below that; records and fragment starts are grown before the kernels that
// write them; a slot index is masked by the table size; a store into the output lies inside [0, out_bytes).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <string>

#include "../../include/defuse_cmp.h"
#include "../../include/defuse_dsa.h"
#include "hip_host.hpp"
#include "rec_shared.hpp"
#include "txt_shared.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using hiphost::grow_keep;
using hiphost::Keep;

thread_local std::string g_cmpt_err;

#define CMPT_HIP(call) HIPHOST_TRY(g_cmpt_err, call)
#define CMPT_FAIL(code, ...) hiphost::fail(g_cmpt_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;       // a slot nobody has claimed
constexpr uint32_t KNOWN = 0x80000000u;       // slot: a name of an earlier piece, its index below; per line: the same instead of a slot
constexpr int64_t MAX_NAMES = (int64_t)1 << 28;      // CMP_META has 28 bits for the reference index
constexpr int64_t MAX_RECORDS = 0xFFFFFFFFll;        // frag_start is uint32 and closed by n_records

// what the host reads between the stages
struct Summary {
    uint32_t stop;              // in: NONE; the lowest stopping line of the piece
    uint32_t stop_kind;
    int64_t stop_start, stop_len;               // that line in the piece's text
    int64_t last_start, last_len;               // field 0 of the piece's last line
    uint32_t table_full, pad_;
};

struct Dict {
    const uint8_t* bytes;
    const int64_t* off;         // n + 1
    int64_t n;
};

// where field 0 of line i ends: at its first tab, or at the line's end
__device__ inline int64_t field0_end(const Lines& L, int64_t i)
{
    const int64_t t0 = first_tab_rank(L, i), t1 = end_tab_rank(L, i);
    return (t1 > t0 && t0 >= 0 && t1 <= L.n_tab) ? (int64_t)L.tab_pos[t0] : line_end(L, i);
}

// field 2 of a line with at least three tabs
__device__ inline void name_of(const Lines& L, int64_t i, int64_t& begin, int64_t& n)
{
    const uint32_t* __restrict__ tp = L.tab_pos + first_tab_rank(L, i);
    begin = (int64_t)tp[1] + 1;
    n = (int64_t)tp[2] - begin;
}

__device__ inline bool same_bytes(const uint8_t* __restrict__ a, int64_t na, const uint8_t* __restrict__ b, int64_t nb)
{
    if (na != nb) return false;
    for (int64_t k = 0; k < na; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

// One lane per line (tools/AlignmentStream.cpp:156-221, in the order of include/defuse_cmp.h).  Lines behind a stop are
// parsed like the others; the host passes them over.
__global__ __launch_bounds__(BLOCK) void k_cmpt_lines(Lines L, int64_t n_lines, const uint8_t* __restrict__ carry, int64_t carry_len,
                                                      cmp_record* __restrict__ recs, uint8_t* __restrict__ kind_of, uint32_t* __restrict__ starts,
                                                      Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_lines) return;
    const uint8_t* __restrict__ text = L.text;
    const int64_t s = line_start(L, i), e = line_end(L, i);
    const int64_t t0 = first_tab_rank(L, i), t1 = end_tab_rank(L, i);
    int kind = 0;
    uint32_t head = 0;
    cmp_record a{0, 0, 0, 0};
    if (e <= s) kind = CMPT_EMPTY_LINE;
    else if (t1 - t0 < 5 || t0 < 0 || t1 > L.n_tab) kind = CMPT_FORMAT;
    else {
        const uint32_t* __restrict__ tp = L.tab_pos + t0;
        const int64_t p0 = tp[0], p1 = tp[1], p2 = tp[2], p3 = tp[3], p4 = tp[4];
        const int64_t p5 = t1 - t0 >= 6 ? (int64_t)tp[5] : e;
        int frag = 0, start = 0, end = 0;
        if (!field_int(text + s, p0 - s, frag)) kind = CMPT_BAD_FRAGMENT;
        else if (!field_int(text + p3 + 1, p4 - p3 - 1, start) || !field_int(text + p4 + 1, p5 - p4 - 1, end)) kind = CMPT_BAD_POSITION;
        else {
            const uint32_t read_end = (p1 - p0 - 1 == 1 && text[p0 + 1] == '1') ? 0u : 1u;
            const uint32_t strand = (p3 - p2 - 1 == 1 && text[p2 + 1] == '-') ? 1u : 0u;
            a = cmp_record{frag, start, end, CMP_META(0, strand, read_end)};
            if (i == 0) head = (carry_len < 0 || !same_bytes(text + s, p0 - s, carry, carry_len)) ? 1u : 0u;
            else {
                const int64_t ps = line_start(L, i - 1);
                head = same_bytes(text + s, p0 - s, text + ps, field0_end(L, i - 1) - ps) ? 0u : 1u;
            }
        }
    }
    if (kind) atomicMin(&sum->stop, (uint32_t)i);
    recs[i] = a;
    kind_of[i] = (uint8_t)kind;
    starts[i] = head;
}

// one thread: the stopping line's kind and place, and field 0 of the last line (what the next piece compares with)
__global__ void k_cmpt_after(Lines L, int64_t n_lines, const uint8_t* __restrict__ kind_of, Summary* __restrict__ sum)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t g = (int64_t)sum->stop;
    if (g < n_lines) {
        sum->stop_kind = kind_of[g];
        sum->stop_start = line_start(L, g);
        sum->stop_len = line_end(L, g) - line_start(L, g);
    }
    sum->last_start = line_start(L, n_lines - 1);
    sum->last_len = field0_end(L, n_lines - 1) - sum->last_start;
}

__device__ inline uint32_t hash_bytes(const uint8_t* __restrict__ p, int64_t n)
{
    uint32_t h = 2166136261u;                  // FNV-1a
    for (int64_t k = 0; k < n; ++k) h = (h ^ p[k]) * 16777619u;
    return h ^ (h >> 15);
}

// One lane per line before the stop: its name's slot (file comment).  where[g] = KNOWN | index for a name of an earlier
// piece, else the slot; NONE if the table is full (the host then refuses the piece).
__global__ __launch_bounds__(BLOCK) void k_cmpt_probe(Lines L, int64_t n_valid, Dict D, uint32_t* __restrict__ slot, uint32_t* __restrict__ first,
                                                      uint32_t mask, uint32_t* __restrict__ where, Summary* __restrict__ sum)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_valid) return;
    const uint8_t* __restrict__ text = L.text;
    int64_t b, n;
    name_of(L, g, b, n);
    uint32_t s = hash_bytes(text + b, n) & mask;
    uint32_t w = NONE;
    for (uint64_t tries = 0; tries <= (uint64_t)mask; ++tries, s = (s + 1) & mask) {
        uint32_t v = __hip_atomic_load(&slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == EMPTY) {
            const uint32_t old = atomicCAS(&slot[s], EMPTY, (uint32_t)g);
            v = old == EMPTY ? (uint32_t)g : old;
        }
        if (v & KNOWN) {
            const int64_t id = (int64_t)(v & ~KNOWN);
            if (id < D.n && same_bytes(text + b, n, D.bytes + D.off[id], D.off[id + 1] - D.off[id])) { w = v; break; }
        } else if ((int64_t)v < n_valid) {
            int64_t rb, rn;
            name_of(L, (int64_t)v, rb, rn);
            if (same_bytes(text + b, n, text + rb, rn)) {
                if (first[s] > (uint32_t)g) atomicMin(&first[s], (uint32_t)g);
                w = s;
                break;
            }
        }
    }
    if (w == NONE) atomicOr(&sum->table_full, 1u);
    where[g] = w;
}

// the line that is the first of a new name, and that name's length
__global__ __launch_bounds__(BLOCK) void k_cmpt_rank(Lines L, int64_t n_valid, const uint32_t* __restrict__ where, const uint32_t* __restrict__ first,
                                                     uint32_t* __restrict__ is_new, uint32_t* __restrict__ new_len)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g > n_valid) return;
    uint32_t f = 0, len = 0;
    if (g < n_valid) {
        const uint32_t w = where[g];
        if (!(w & KNOWN) && first[w] == (uint32_t)g) {
            int64_t b, n;
            name_of(L, g, b, n);
            f = 1;
            len = (uint32_t)n;
        }
    }
    is_new[g] = f;              // (element n_valid is 0: the sums' last outputs are the totals)
    new_len[g] = len;
}

// The first line of a new name appends it: index = names before this piece + rank, bytes behind those that are there.
__global__ __launch_bounds__(BLOCK) void k_cmpt_assign(Lines L, int64_t n_valid, const uint32_t* __restrict__ where, const uint32_t* __restrict__ is_new,
                                                       const uint32_t* __restrict__ rank, const u64* __restrict__ byte_off, int64_t n_old, int64_t bytes_old,
                                                       int64_t n_new, int64_t bytes_new, uint32_t* __restrict__ slot, uint8_t* __restrict__ name_bytes,
                                                       int64_t* __restrict__ name_off)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_valid || !is_new[g]) return;
    int64_t b, n;
    name_of(L, g, b, n);
    const int64_t r = (int64_t)rank[g], at = (int64_t)byte_off[g];
    if (r >= n_new || at + n > bytes_new) return;
    for (int64_t k = 0; k < n; ++k) name_bytes[bytes_old + at + k] = L.text[b + k];
    name_off[n_old + r + 1] = bytes_old + at + n;
    slot[where[g]] = KNOWN | (uint32_t)(n_old + r);
}

// every record's reference index, and the fragment starts
__global__ __launch_bounds__(BLOCK) void k_cmpt_refs(int64_t n_valid, const uint32_t* __restrict__ where, const uint32_t* __restrict__ slot,
                                                     const uint32_t* __restrict__ starts, const uint32_t* __restrict__ frag_rank, int64_t n_new_frags,
                                                     int64_t rec_base, cmp_record* __restrict__ recs, uint32_t* __restrict__ frag_start)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_valid) return;
    const uint32_t w = where[g];
    const uint32_t id = ((w & KNOWN) ? w : slot[w]) & 0x0FFFFFFFu;
    recs[g].meta = (recs[g].meta & ~0x0FFFFFFFu) | id;
    if (starts[g] && (int64_t)frag_rank[g] < n_new_frags) frag_start[frag_rank[g]] = (uint32_t)(rec_base + g);
}

__global__ void k_cmpt_close(uint32_t* __restrict__ frag_start, int64_t n_fragments, int64_t n_records)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) frag_start[n_fragments] = (uint32_t)n_records;
}

// ---- the printer ----------------------------------------------------------------------------------------------------------

// One lane per output line q = 2 * row + end: its length; the lowest row with a ref outside the dictionary.
__global__ __launch_bounds__(BLOCK) void k_cmpt_lengths(const cmp_row* __restrict__ rows, int64_t n_out, Dict D, uint32_t* __restrict__ len,
                                                        u64* __restrict__ bad_row)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q > n_out) return;
    uint32_t n = 0;
    if (q < n_out) {
        const cmp_row& r = rows[q >> 1];
        const int ce = (int)(q & 1);
        const int64_t ref = r.ref[ce];
        if (ref < 0 || ref >= D.n) atomicMin(bad_row, (u64)(q >> 1));
        else
            n = (uint32_t)(rec_field_length(r.cluster_id) + 2 + rec_field_length(r.fragment[ce]) + rec_field_length(r.read_end[ce]) +
                           (D.off[ref + 1] - D.off[ref]) + 1 + 2 + rec_field_length(r.start[ce]) + rec_field_length(r.end[ce]));
    }
    len[q] = n;                 // (element n_out is 0: the sum's last output is the total)
}

__global__ __launch_bounds__(BLOCK) void k_cmpt_write(const cmp_row* __restrict__ rows, int64_t n_out, Dict D, const uint32_t* __restrict__ len,
                                                      const u64* __restrict__ dst, uint8_t* __restrict__ out, int64_t out_bytes)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_out) return;
    const cmp_row& r = rows[q >> 1];
    const int ce = (int)(q & 1);
    const int64_t ref = r.ref[ce];
    const int64_t at = (int64_t)dst[q];
    if (ref < 0 || ref >= D.n || at < 0 || at + (int64_t)len[q] > out_bytes) return;
    uint8_t* __restrict__ o = out + at;
    o += rec_write_field(r.cluster_id, o);
    *o++ = (uint8_t)('0' + ce);
    *o++ = '\t';
    o += rec_write_field(r.fragment[ce], o);
    o += rec_write_field(r.read_end[ce], o);
    const uint8_t* __restrict__ name = D.bytes + D.off[ref];
    const int64_t nn = D.off[ref + 1] - D.off[ref];
    for (int64_t k = 0; k < nn; ++k) o[k] = name[k];
    o += nn;
    *o++ = '\t';
    *o++ = r.strand[ce] == 0 ? '+' : '-';
    *o++ = '\t';
    o += rec_write_field(r.start[ce], o);
    o += rec_write_field(r.end[ce], o, '\n');
}

}  // namespace

struct cmpt_ctx {
    int device = -1;
    int64_t max_names = 0;
    uint32_t table_size = 0;
    hiphost::Stream st;
    hiphost::Event ev[10];
    cmpt_timing timing{};
    // the stream
    bool stopped = false, failed = false;
    cmpt_result res{};
    int64_t n_bytes = 0, n_name_bytes = 0, carry_len = -1;
    DeviceBuffer<cmp_record> recs;
    DeviceBuffer<uint32_t> frag_start;
    DeviceBuffer<uint8_t> name_bytes, carry;
    DeviceBuffer<int64_t> name_off;
    DeviceBuffer<uint32_t> slot, first;
    // a piece
    DeviceBuffer<uint8_t, GrowSize> text, kind_of;
    TextScratch scratch;
    TextTables tables;
    DeviceBuffer<u64, GrowSize> byte_off;
    DeviceBuffer<uint32_t, GrowSize> starts, frag_rank, where, is_new, new_len, rank;
    DeviceBuffer<Summary> summary;
    // the printer
    DeviceBuffer<cmp_row, GrowSize> rows;
    DeviceBuffer<uint32_t, GrowSize> out_len;
    DeviceBuffer<u64, GrowSize> out_dst;
    DeviceBuffer<u64> bad_row;
    DeviceBuffer<uint8_t, GrowSize> out;
    int64_t out_bytes = 0;
};

namespace {

int reset_stream(cmpt_ctx* c)
{
    hipStream_t st = c->st;
    CMPT_HIP(c->slot.reserve(c->table_size));
    CMPT_HIP(c->first.reserve(c->table_size));
    CMPT_HIP(c->name_off.reserve(64));
    CMPT_HIP(c->frag_start.reserve(64));
    CMPT_HIP(hipMemsetAsync(c->slot.p, 0xFF, (size_t)c->table_size * sizeof(uint32_t), st));
    CMPT_HIP(hipMemsetAsync(c->first.p, 0xFF, (size_t)c->table_size * sizeof(uint32_t), st));
    CMPT_HIP(hipMemsetAsync(c->name_off.p, 0, sizeof(int64_t), st));
    CMPT_HIP(hipMemsetAsync(c->frag_start.p, 0, sizeof(uint32_t), st));
    CMPT_HIP(hipStreamSynchronize(st));
    c->stopped = c->failed = false;
    c->res = cmpt_result{};
    c->n_bytes = c->n_name_bytes = 0;
    c->carry_len = -1;
    c->out_bytes = 0;
    c->timing = cmpt_timing{};
    return DSA_OK;
}

// One piece of `len` > 0 bytes; `on_device`: text is device memory.  With final = 0 the host form brings whole lines only, the
// device form may end in an open line, which is then no line.  *consumed: what was taken.
int add_piece(cmpt_ctx* c, const uint8_t* text, int64_t len, bool on_device, bool final, int64_t* consumed)
{
    CMPT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CMPT_HIP(c->text.reserve(padded_size(len)));
    CMPT_HIP(c->summary.reserve(1));
    Totals tot{};
    if (const int rc = text_upload_count<true>(g_cmpt_err, c->scratch, c->text.p, text, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, len, c->ev[0],
                                               c->ev[1], st, tot))
        return rc;
    const int64_t n_nl = (int64_t)tot.n_nl;
    const bool open_end = tot.last != '\n';
    const int64_t n_lines = n_nl + (open_end && final ? 1 : 0);
    CMPT_HIP(c->tables.reserve(tot));
    const Lines L = c->tables.place<true>(c->scratch, c->text.p, len, tot, st);
    CMPT_HIP(hipEventRecord(c->ev[2], st));
    *consumed = len;
    if (open_end && !final) {                                   // (the device form only)
        uint32_t last_nl = 0;
        if (n_nl) CMPT_HIP(hipMemcpyAsync(&last_nl, c->tables.nl_pos.p + (n_nl - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CMPT_HIP(hipStreamSynchronize(st));
        *consumed = n_nl ? (int64_t)last_nl + 1 : 0;
    }
    c->timing.text_bytes += *consumed;
    c->timing.n_pieces += 1;
    if (n_lines == 0) {
        CMPT_HIP(hipStreamSynchronize(st));
        CMPT_HIP(hipGetLastError());
        c->timing.upload_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
        c->timing.tables_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
        c->n_bytes += *consumed;
        return DSA_OK;
    }
    const int64_t rec_base = c->res.n_records, frag_base = c->res.n_fragments, n_old = c->res.n_names, bytes_old = c->n_name_bytes;
    const unsigned gl = grid_of(n_lines + 1);

    // lines (the records of all lines of the piece have room: a stop is not known yet)
    if (rec_base + n_lines > MAX_RECORDS) return CMPT_FAIL(DSA_E_LIMIT, "more than 2^32 - 1 alignment records");
    CMPT_HIP(grow_keep(c->recs, Keep{(size_t)rec_base}, (size_t)(rec_base + n_lines), st));
    CMPT_HIP(c->kind_of.reserve((size_t)n_lines + 1));
    for (auto* b : {&c->starts, &c->frag_rank, &c->where, &c->is_new, &c->new_len, &c->rank}) CMPT_HIP(b->reserve((size_t)n_lines + 1));
    CMPT_HIP(c->byte_off.reserve((size_t)n_lines + 1));
    Summary sum{};
    sum.stop = NONE;
    CMPT_HIP(hipMemcpyAsync(c->summary.p, &sum, sizeof(Summary), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cmpt_lines, dim3(gl), dim3(BLOCK), 0, st, L, n_lines, (const uint8_t*)c->carry.p, c->carry_len, c->recs.p + rec_base, c->kind_of.p,
                       c->starts.p, c->summary.p);
    hipLaunchKernelGGL(k_cmpt_after, dim3(1), dim3(64), 0, st, L, n_lines, (const uint8_t*)c->kind_of.p, c->summary.p);
    CMPT_HIP(hipEventRecord(c->ev[3], st));
    CMPT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipStreamSynchronize(st));
    CMPT_HIP(hipGetLastError());
    const bool stop = (int64_t)sum.stop < n_lines;
    const int64_t n_valid = stop ? (int64_t)sum.stop : n_lines;
    if (stop && (sum.stop_kind < CMPT_EMPTY_LINE || sum.stop_kind > CMPT_BAD_POSITION || sum.stop_start < 0 || sum.stop_len < 0 || sum.stop_start + sum.stop_len > len))
        return CMPT_FAIL(DSA_E_DEVICE, "internal: stop of kind %u at [%lld, +%lld) of %lld bytes", sum.stop_kind, (long long)sum.stop_start, (long long)sum.stop_len, (long long)len);
    if (sum.last_start < 0 || sum.last_len < 0 || sum.last_start + sum.last_len > len)
        return CMPT_FAIL(DSA_E_DEVICE, "internal: the last line's first field at [%lld, +%lld) of %lld bytes", (long long)sum.last_start, (long long)sum.last_len, (long long)len);

    int64_t n_new_frags = 0, n_new = 0, bytes_new = 0;
    if (n_valid) {
        const unsigned gv = grid_of(n_valid + 1);
        // layout, first half: the fragments' ranks
        CMPT_HIP(hipEventRecord(c->ev[4], st));
        CMPT_HIP(hipMemsetAsync(c->starts.p + n_valid, 0, sizeof(uint32_t), st));
        CMPT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceScan::ExclusiveSum(w, wb, c->starts.p, c->frag_rank.p, (int)(n_valid + 1), st);
        }));
        CMPT_HIP(hipEventRecord(c->ev[5], st));
        // names
        const Dict D{c->name_bytes.p, c->name_off.p, n_old};
        hipLaunchKernelGGL(k_cmpt_probe, dim3(gv), dim3(BLOCK), 0, st, L, n_valid, D, c->slot.p, c->first.p, c->table_size - 1, c->where.p, c->summary.p);
        hipLaunchKernelGGL(k_cmpt_rank, dim3(gv), dim3(BLOCK), 0, st, L, n_valid, (const uint32_t*)c->where.p, (const uint32_t*)c->first.p, c->is_new.p,
                           c->new_len.p);
        CMPT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceScan::ExclusiveSum(w, wb, c->is_new.p, c->rank.p, (int)(n_valid + 1), st);
        }));
        hipcub::TransformInputIterator<u64, Widen, const uint32_t*> lengths(c->new_len.p, Widen());
        CMPT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceScan::ExclusiveSum(w, wb, lengths, c->byte_off.p, (int)(n_valid + 1), st);
        }));
        CMPT_HIP(hipEventRecord(c->ev[6], st));
        uint32_t tot_frags = 0, tot_new = 0;
        u64 tot_bytes = 0;
        CMPT_HIP(hipMemcpyAsync(&tot_frags, c->frag_rank.p + n_valid, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CMPT_HIP(hipMemcpyAsync(&tot_new, c->rank.p + n_valid, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CMPT_HIP(hipMemcpyAsync(&tot_bytes, c->byte_off.p + n_valid, sizeof(u64), hipMemcpyDeviceToHost, st));
        CMPT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
        CMPT_HIP(hipStreamSynchronize(st));
        CMPT_HIP(hipGetLastError());
        n_new_frags = tot_frags;
        n_new = tot_new;
        bytes_new = (int64_t)tot_bytes;
        if (sum.table_full || n_old + n_new > c->max_names)
            return CMPT_FAIL(DSA_E_LIMIT, "more than %lld distinct reference names (max_names of cmpt_create)", (long long)c->max_names);
        if (n_new_frags > n_valid || n_new > n_valid || bytes_new > len)
            return CMPT_FAIL(DSA_E_DEVICE, "internal: %lld fragments, %lld names of %lld bytes in %lld lines", (long long)n_new_frags, (long long)n_new,
                             (long long)bytes_new, (long long)n_valid);
        CMPT_HIP(grow_keep(c->name_bytes, Keep{(size_t)bytes_old}, (size_t)(bytes_old + bytes_new), st));
        CMPT_HIP(grow_keep(c->name_off, Keep{(size_t)n_old + 1}, (size_t)(n_old + n_new + 1), st));
        CMPT_HIP(grow_keep(c->frag_start, Keep{(size_t)frag_base + 1}, (size_t)(frag_base + n_new_frags + 1), st));
        CMPT_HIP(hipEventRecord(c->ev[7], st));
        hipLaunchKernelGGL(k_cmpt_assign, dim3(gv), dim3(BLOCK), 0, st, L, n_valid, (const uint32_t*)c->where.p, (const uint32_t*)c->is_new.p,
                           (const uint32_t*)c->rank.p, (const u64*)c->byte_off.p, n_old, bytes_old, n_new, bytes_new, c->slot.p, c->name_bytes.p, c->name_off.p);
        CMPT_HIP(hipEventRecord(c->ev[8], st));
        // layout, second half
        hipLaunchKernelGGL(k_cmpt_refs, dim3(gv), dim3(BLOCK), 0, st, n_valid, (const uint32_t*)c->where.p, (const uint32_t*)c->slot.p,
                           (const uint32_t*)c->starts.p, (const uint32_t*)c->frag_rank.p, n_new_frags, rec_base, c->recs.p + rec_base, c->frag_start.p + frag_base);
        hipLaunchKernelGGL(k_cmpt_close, dim3(1), dim3(64), 0, st, c->frag_start.p, frag_base + n_new_frags, rec_base + n_valid);
    }
    if (!stop) {                                                // what the next piece's first line compares with
        CMPT_HIP(c->carry.reserve((size_t)sum.last_len));
        if (sum.last_len) CMPT_HIP(hipMemcpyAsync(c->carry.p, c->text.p + sum.last_start, (size_t)sum.last_len, hipMemcpyDeviceToDevice, st));
    }
    CMPT_HIP(hipEventRecord(c->ev[9], st));
    CMPT_HIP(hipStreamSynchronize(st));
    CMPT_HIP(hipGetLastError());
    c->timing.upload_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.tables_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.lines_ms += hiphost::elapsed(c->ev[2], c->ev[3]);
    if (n_valid) {
        c->timing.names_ms += hiphost::elapsed(c->ev[5], c->ev[6]) + hiphost::elapsed(c->ev[7], c->ev[8]);
        c->timing.layout_ms += hiphost::elapsed(c->ev[4], c->ev[5]) + hiphost::elapsed(c->ev[8], c->ev[9]);
    }
    if (stop) {
        c->stopped = true;
        c->res.stop_kind = (int32_t)sum.stop_kind;
        c->res.stop_line = c->res.n_lines + n_valid + 1;
        c->res.stop_offset = c->n_bytes + sum.stop_start;
        c->res.stop_len = sum.stop_len;
    } else c->carry_len = sum.last_len;
    c->res.n_lines += n_valid + (stop ? 1 : 0);
    c->res.n_records += n_valid;
    c->res.n_fragments += n_new_frags;
    c->res.n_names += n_new;
    c->n_name_bytes += bytes_new;
    c->n_bytes += *consumed;
    return DSA_OK;
}

int add(cmpt_ctx* c, const uint8_t* text, int64_t len, int32_t final, cmpt_result* result, bool on_device, const char* who)
{
    if (!result) return CMPT_FAIL(DSA_E_ARG, "%s: no result", who);
    *result = cmpt_result{};
    if (len < 0) return CMPT_FAIL(DSA_E_ARG, "%s: negative length (%lld)", who, (long long)len);
    if (len > (int64_t)INT32_MAX) return CMPT_FAIL(DSA_E_LIMIT, "%s: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", who, (long long)len);
    if (len && !text) return CMPT_FAIL(DSA_E_ARG, "%s: null pointer with non-zero size", who);
    if (final != 0 && final != 1) return CMPT_FAIL(DSA_E_ARG, "%s: final %d is not 0 or 1", who, final);
    if (!c) return CMPT_FAIL(DSA_E_ARG, "%s: no ctx", who);
    if (c->failed) return CMPT_FAIL(DSA_E_ARG, "%s after a failed call: cmpt_begin starts the next stream", who);
    if (!on_device && !final) len = whole_lines(text, len);
    int64_t consumed = len;
    if (len && !c->stopped) {
        c->out_bytes = 0;
        const int rc = add_piece(c, text, len, on_device, final != 0, &consumed);
        if (rc != DSA_OK) {
            (void)hipStreamSynchronize(c->st);                 // nothing of a refused call is in flight when it returns
            c->failed = true;
            return rc;
        }
    }
    *result = c->res;
    result->consumed = consumed;
    return DSA_OK;
}

int print_rows(cmpt_ctx* c, const cmp_row* rows, int64_t n_rows, cmpt_print_result* r)
{
    CMPT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    r->n_rows = n_rows;
    r->bad_row = -1;
    if (n_rows == 0) return DSA_OK;
    const int64_t n_out = 2 * n_rows;
    const unsigned gl = grid_of(n_out + 1);
    const Dict D{c->name_bytes.p, c->name_off.p, c->res.n_names};
    CMPT_HIP(c->out_len.reserve((size_t)n_out + 1));
    CMPT_HIP(c->out_dst.reserve((size_t)n_out + 1));
    CMPT_HIP(c->bad_row.reserve(1));
    CMPT_HIP(hipMemsetAsync(c->bad_row.p, 0xFF, sizeof(u64), st));
    CMPT_HIP(hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_cmpt_lengths, dim3(gl), dim3(BLOCK), 0, st, rows, n_out, D, c->out_len.p, c->bad_row.p);
    hipcub::TransformInputIterator<u64, Widen, const uint32_t*> lengths(c->out_len.p, Widen());     // 32-bit lengths, a 64-bit sum
    CMPT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, lengths, c->out_dst.p, (int)(n_out + 1), st); }));
    CMPT_HIP(hipEventRecord(c->ev[1], st));
    u64 bad = 0, total = 0;
    CMPT_HIP(hipMemcpyAsync(&bad, c->bad_row.p, sizeof(u64), hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipMemcpyAsync(&total, c->out_dst.p + n_out, sizeof(u64), hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipStreamSynchronize(st));
    CMPT_HIP(hipGetLastError());
    c->timing.lengths_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    if (bad != ~0ull) {
        r->bad_row = (int64_t)bad;
        return CMPT_FAIL(DSA_E_ARG, "row %lld has a reference index outside the %lld names of the stream", (long long)bad, (long long)c->res.n_names);
    }
    CMPT_HIP(c->out.reserve((size_t)total));
    hipLaunchKernelGGL(k_cmpt_write, dim3(gl), dim3(BLOCK), 0, st, rows, n_out, D, (const uint32_t*)c->out_len.p, (const u64*)c->out_dst.p, c->out.p, (int64_t)total);
    CMPT_HIP(hipEventRecord(c->ev[2], st));
    CMPT_HIP(hipStreamSynchronize(st));
    CMPT_HIP(hipGetLastError());
    c->timing.write_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->out_bytes = r->text_bytes = c->timing.out_bytes = (int64_t)total;
    return DSA_OK;
}

int print_entry(cmpt_ctx* c, const cmp_row* rows, int64_t n_rows, cmpt_print_result* r, bool on_device, const char* who)
{
    if (!r) return CMPT_FAIL(DSA_E_ARG, "%s: no result", who);
    *r = cmpt_print_result{0, 0, -1};
    if (n_rows < 0) return CMPT_FAIL(DSA_E_ARG, "%s: negative row count (%lld)", who, (long long)n_rows);
    if (n_rows > (int64_t)INT32_MAX / 2 - 1) return CMPT_FAIL(DSA_E_LIMIT, "%s: more than 2^30 - 2 rows in one call: print in rounds", who);
    if (n_rows && !rows) return CMPT_FAIL(DSA_E_ARG, "%s: null pointer with a non-zero count", who);
    if (!c) return CMPT_FAIL(DSA_E_ARG, "%s: no ctx", who);
    if (c->failed) return CMPT_FAIL(DSA_E_ARG, "%s after a failed call: cmpt_begin starts the next stream", who);
    c->out_bytes = 0;
    c->timing.lengths_ms = c->timing.write_ms = c->timing.download_ms = 0.f;
    c->timing.out_bytes = 0;
    if (n_rows && !on_device) {
        CMPT_HIP(hipSetDevice(c->device));
        CMPT_HIP(c->rows.reserve((size_t)n_rows));
        CMPT_HIP(hipMemcpyAsync(c->rows.p, rows, (size_t)n_rows * sizeof(cmp_row), hipMemcpyHostToDevice, c->st));
        rows = c->rows.p;
    }
    const int rc = print_rows(c, rows, n_rows, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->out_bytes = 0;
    }
    return rc;
}

}  // namespace

extern "C" {

const char* cmpt_last_error(void) { return g_cmpt_err.c_str(); }

int cmpt_create(int device, int64_t max_names, cmpt_ctx** out)
{
    if (!out) return CMPT_FAIL(DSA_E_ARG, "cmpt_create: no output");
    *out = nullptr;
    if (max_names < 1 || max_names > MAX_NAMES) return CMPT_FAIL(DSA_E_ARG, "cmpt_create: max_names %lld is outside [1, 2^28]", (long long)max_names);
    if (hiphost::check_device(device, &g_cmpt_err)) return DSA_E_DEVICE;
    CMPT_HIP(hipSetDevice(device));
    cmpt_ctx* c = new cmpt_ctx();
    c->device = device;
    c->max_names = max_names;
    c->table_size = 2;
    while ((int64_t)c->table_size < 2 * max_names) c->table_size *= 2;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return CMPT_FAIL(DSA_E_DEVICE, "cannot create a stream or an event");
    }
    const int rc = reset_stream(c);
    if (rc != DSA_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return DSA_OK;
}

void cmpt_destroy(cmpt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int cmpt_begin(cmpt_ctx* c)
{
    if (!c) return CMPT_FAIL(DSA_E_ARG, "cmpt_begin: no ctx");
    CMPT_HIP(hipSetDevice(c->device));
    CMPT_HIP(hipStreamSynchronize(c->st));
    return reset_stream(c);
}

int cmpt_add(cmpt_ctx* c, const uint8_t* text, int64_t len, int32_t final, cmpt_result* result)
{
    return add(c, text, len, final, result, false, "cmpt_add");
}

int cmpt_add_device(cmpt_ctx* c, const uint8_t* text_device, int64_t len, int32_t final, cmpt_result* result)
{
    return add(c, text_device, len, final, result, true, "cmpt_add_device");
}

int cmpt_view(const cmpt_ctx* c, cmpt_device* out)
{
    if (!c || !out) return CMPT_FAIL(DSA_E_ARG, "cmpt_view: no %s", !c ? "ctx" : "output");
    if (c->failed) return CMPT_FAIL(DSA_E_ARG, "cmpt_view after a failed call: cmpt_begin starts the next stream");
    *out = cmpt_device{c->recs.p, c->frag_start.p, c->name_bytes.p, c->name_off.p, c->res.n_records, c->res.n_fragments, c->res.n_names, c->n_name_bytes,
                       c->device, 0};
    return DSA_OK;
}

int cmpt_fetch(cmpt_ctx* c, cmp_record* records, int64_t record_cap, uint32_t* frag_start, int64_t frag_cap)
{
    if (!c) return CMPT_FAIL(DSA_E_ARG, "cmpt_fetch: no ctx");
    if (c->failed) return CMPT_FAIL(DSA_E_ARG, "cmpt_fetch after a failed call: cmpt_begin starts the next stream");
    if (record_cap < 0 || frag_cap < 0) return CMPT_FAIL(DSA_E_ARG, "cmpt_fetch: negative capacity");
    if (records && record_cap < c->res.n_records) return CMPT_FAIL(DSA_E_CAPACITY, "cmpt_fetch: %lld records, room for %lld", (long long)c->res.n_records, (long long)record_cap);
    if (frag_start && frag_cap < c->res.n_fragments + 1)
        return CMPT_FAIL(DSA_E_CAPACITY, "cmpt_fetch: %lld fragment starts and their end, room for %lld", (long long)c->res.n_fragments, (long long)frag_cap);
    CMPT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    if (records && c->res.n_records) CMPT_HIP(hipMemcpyAsync(records, c->recs.p, (size_t)c->res.n_records * sizeof(cmp_record), hipMemcpyDeviceToHost, st));
    if (frag_start) CMPT_HIP(hipMemcpyAsync(frag_start, c->frag_start.p, (size_t)(c->res.n_fragments + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipStreamSynchronize(st));
    return DSA_OK;
}

int cmpt_names_fetch(cmpt_ctx* c, uint8_t* bytes, int64_t byte_cap, int64_t* off, int64_t off_cap)
{
    if (!c) return CMPT_FAIL(DSA_E_ARG, "cmpt_names_fetch: no ctx");
    if (c->failed) return CMPT_FAIL(DSA_E_ARG, "cmpt_names_fetch after a failed call: cmpt_begin starts the next stream");
    if (byte_cap < 0 || off_cap < 0) return CMPT_FAIL(DSA_E_ARG, "cmpt_names_fetch: negative capacity");
    if (bytes && byte_cap < c->n_name_bytes) return CMPT_FAIL(DSA_E_CAPACITY, "cmpt_names_fetch: %lld bytes of names, room for %lld", (long long)c->n_name_bytes, (long long)byte_cap);
    if (off && off_cap < c->res.n_names + 1) return CMPT_FAIL(DSA_E_CAPACITY, "cmpt_names_fetch: %lld names and their end, room for %lld", (long long)c->res.n_names, (long long)off_cap);
    CMPT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    if (bytes && c->n_name_bytes) CMPT_HIP(hipMemcpyAsync(bytes, c->name_bytes.p, (size_t)c->n_name_bytes, hipMemcpyDeviceToHost, st));
    if (off) CMPT_HIP(hipMemcpyAsync(off, c->name_off.p, (size_t)(c->res.n_names + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipStreamSynchronize(st));
    return DSA_OK;
}

int cmpt_print_rows(cmpt_ctx* c, const cmp_row* rows, int64_t n_rows, cmpt_print_result* result)
{
    return print_entry(c, rows, n_rows, result, false, "cmpt_print_rows");
}

int cmpt_print_rows_device(cmpt_ctx* c, const cmp_row* rows_device, int64_t n_rows, cmpt_print_result* result)
{
    return print_entry(c, rows_device, n_rows, result, true, "cmpt_print_rows_device");
}

int cmpt_text_fetch(cmpt_ctx* c, uint8_t* buf, int64_t cap, int64_t* n_bytes)
{
    if (!n_bytes) return CMPT_FAIL(DSA_E_ARG, "cmpt_text_fetch: no place for the size");
    *n_bytes = 0;
    if (cap < 0) return CMPT_FAIL(DSA_E_ARG, "cmpt_text_fetch: negative capacity");
    if (!c) return CMPT_FAIL(DSA_E_ARG, "cmpt_text_fetch: no ctx");
    *n_bytes = c->out_bytes;
    if (c->out_bytes > cap) return CMPT_FAIL(DSA_E_CAPACITY, "cmpt_text_fetch: %lld bytes of text, room for %lld", (long long)c->out_bytes, (long long)cap);
    if (c->out_bytes == 0) return DSA_OK;
    if (!buf) return CMPT_FAIL(DSA_E_ARG, "cmpt_text_fetch: null buffer");
    CMPT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CMPT_HIP(hipEventRecord(c->ev[3], st));
    CMPT_HIP(hipMemcpyAsync(buf, c->out.p, (size_t)c->out_bytes, hipMemcpyDeviceToHost, st));
    CMPT_HIP(hipEventRecord(c->ev[4], st));
    CMPT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms += hiphost::elapsed(c->ev[3], c->ev[4]);
    return DSA_OK;
}

int cmpt_get_timing(const cmpt_ctx* c, cmpt_timing* out)
{
    if (!c || !out) return CMPT_FAIL(DSA_E_ARG, "cmpt_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
