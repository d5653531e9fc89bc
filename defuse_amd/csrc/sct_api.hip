// sct_api.hip — the text front and back of the set cover on gfx950 (include/defuse_sc.h, section "cluster text"): the cluster
// file goes up in pieces, ReadClusters and WriteClusters of the reference (tools/Parsers.cpp:23-170) run on the device around
// sc_shared.hpp's set cover, and the filtered cluster file comes down as bytes.
//
// A piece (sct_add) stays in device memory with the positions of its newlines (txt_shared.hpp, without tabs: the three fields
// that matter sit at the start of a line, and a lane scans them from there).  sct_cover then works on all pieces at once; a lane
// finds the piece of its line by a binary search over the pieces' first line numbers, so the number of launches does not grow
// with the number of pieces:
//   parse   k_sct_lines: one lane per line writes (clusterID, fragmentIndex, kind | end-0 flag); the first read stop and the
//           first write stop are atomic minima over the (rare) candidates, the largest end-0 cluster id and fragment and the
//           number of end-0 lines one atomic per workgroup.  These few counts go to the host, which sizes what follows.
//   layout  the end-0 lines' (cluster << 32 | fragment) compacted in file order, a stable radix sort on the cluster half, lower bounds:
//           clusters[id] in file order, in CSR form.
//   cover   sc_cover_device.
//   select  a histogram over owner[] gives the clusters' solution sizes, k_sct_keep a flag and an output length per line,
//           k_sct_heads the heads of the runs of adjacent kept lines (inside a piece, and cut every RUN_LINES lines so that no
//           run grows with the file); two exclusive sums give every line its output offset (64 bit) and every head its rank.
//   gather  k_sct_runs: a head lane walks to the end of its run and writes its record; k_sct_gather copies one run per group of
//           RUN_GROUP lanes with whole-dword stores wherever the output allows (bat_shared.hpp's scheme, the source chosen per
//           run).  The one newline a last line without one gains is a byte store of the lane that wrote the run.
// Every read of a piece's text is below its length or inside the zeroed padding of whole chunks behind it; every per-line array
// is indexed below n_lines; every store into the output lies inside [0, out_bytes).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_sc.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "sc_shared.hpp"
#include "txt_shared.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;

thread_local std::string g_sct_err;

#define SCT_HIP(call) HIPHOST_TRY(g_sct_err, call)
#define SCT_FAIL(code, ...) hiphost::fail(g_sct_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int RUN_LINES = 64;                 // a run of kept lines is cut at every multiple of this inside its piece
constexpr int RUN_GROUP = 16;                 // lanes per run in the gather (measured against 64: profiles/sctext/README.md)
constexpr uint8_t END0 = 8;                   // meta: the kind in bits 0-2, "clusterEnd == 0" in bit 3
static_assert(TEXT_PAD >= batdev::SRC_PAD + CHUNK, "padding");        // k_sct_gather reads the pieces' texts

struct PieceView {
    const uint8_t* text;
    const uint32_t* nl_pos;     // n_nl positions of '\n', ascending
    int64_t len, n_nl, n_lines;
    int64_t line_base;          // lines of the pieces in front
    int64_t base;               // bytes of the pieces in front
};

// what the host reads between the stages, and the two stops (in: NONE)
struct Summary {
    uint32_t rstop, wstop;      // the lowest line (0-based over all pieces) of a read stop / of a negative cluster id
    int32_t max_cid, max_el;    // over the end-0 lines (in: -1)
    uint32_t negative, stop_kind;
    u64 n_members;
    int64_t stop_offset, stop_len;
    u64 n_kept, n_added_nl;
    int64_t out_bytes, n_runs;
};

struct Run {
    int64_t src;                // offset into its piece's text
    int64_t dst;                // offset into the output
    uint32_t len, piece;
};

// the piece that holds line g: the last one whose first line is not behind g (every piece has a line)
__device__ inline int piece_of(const PieceView* __restrict__ pv, int n_pieces, int64_t g)
{
    int lo = 0, hi = n_pieces - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pv[mid].line_base <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline int64_t piece_line_start(const PieceView& P, int64_t i) { return i == 0 ? 0 : (int64_t)P.nl_pos[i - 1] + 1; }
__device__ inline int64_t piece_line_end(const PieceView& P, int64_t i) { return i < P.n_nl ? (int64_t)P.nl_pos[i] : P.len; }

// One lane per line: the three integers and the line's kind (tools/Parsers.cpp:42-71, in that order).
__global__ __launch_bounds__(BLOCK) void k_sct_lines(const PieceView* __restrict__ pv, int n_pieces, int64_t n_lines, int32_t* __restrict__ cid,
                                                     int32_t* __restrict__ frag, uint8_t* __restrict__ meta, uint8_t* __restrict__ member,
                                                     Summary* __restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<int, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp[3];
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    int kind = 0, c = 0, e = 0, f = 0;
    bool is_member = false;
    if (g < n_lines) {
        const PieceView P = pv[piece_of(pv, n_pieces, g)];
        const int64_t i = g - P.line_base;
        const int64_t s0 = piece_line_start(P, i), e0 = piece_line_end(P, i);
        const uint8_t* __restrict__ text = P.text;
        if (e0 <= s0) kind = SCT_EMPTY_LINE;
        else {
            int64_t t1 = s0;
            while (t1 < e0 && text[t1] != '\t') ++t1;
            int64_t t2 = t1 < e0 ? t1 + 1 : e0;
            while (t2 < e0 && text[t2] != '\t') ++t2;
            if (t2 >= e0) kind = SCT_FEW_FIELDS;                  // no second tab
            else {
                int64_t t3 = t2 + 1;
                while (t3 < e0 && text[t3] != '\t') ++t3;
                if (!field_int(text + s0, t1 - s0, c) || !field_int(text + t1 + 1, t2 - t1 - 1, e) || !field_int(text + t2 + 1, t3 - t2 - 1, f))
                    kind = SCT_BAD_INTEGER;
                else if (e == 0 && c < 0) kind = SCT_BAD_CLUSTER_ID;
            }
        }
        is_member = kind == 0 && e == 0;
        cid[g] = c;
        frag[g] = f;
        meta[g] = (uint8_t)(kind | (is_member ? END0 : 0));
        member[g] = is_member ? 1 : 0;
        if (kind) atomicMin(&sum->rstop, (uint32_t)g);
        else if (c < 0) atomicMin(&sum->wstop, (uint32_t)g);      // (an end-0 line with such an id is a read stop)
    }
    const int max_c = Reduce(tmp[0]).Reduce(is_member ? c : -1, hipcub::Max());
    const int max_f = Reduce(tmp[1]).Reduce(is_member ? f : -1, hipcub::Max());
    const int n_mem = Reduce(tmp[2]).Sum(is_member ? 1 : 0);
    const int any_neg = __syncthreads_or(is_member && f < 0);
    if (threadIdx.x == 0 && n_mem) {
        atomicMax(&sum->max_cid, max_c);
        atomicMax(&sum->max_el, max_f);
        atomicAdd(&sum->n_members, (u64)n_mem);
        if (any_neg) atomicOr(&sum->negative, 1u);
    }
}

// one thread: where the stopping line `g` lies in the caller's input, and its kind
__global__ void k_sct_stop(const PieceView* __restrict__ pv, int n_pieces, int64_t g, const uint8_t* __restrict__ meta, int write_stop,
                           Summary* __restrict__ sum)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const PieceView P = pv[piece_of(pv, n_pieces, g)];
    const int64_t i = g - P.line_base;
    const int64_t s0 = piece_line_start(P, i), e0 = piece_line_end(P, i);
    sum->stop_offset = P.base + s0;
    sum->stop_len = e0 - s0;
    sum->stop_kind = write_stop ? (uint32_t)SCT_BAD_CLUSTER_ID : (uint32_t)(meta[g] & 7);
}

// (clusterID << 32 | fragmentIndex) of line i; only end-0 lines are selected, whose ids are not negative
struct PackMember {
    const int32_t* cid;
    const int32_t* frag;
    __host__ __device__ u64 operator()(int64_t i) const { return ((u64)(uint32_t)cid[i] << 32) | (u64)(uint32_t)frag[i]; }
};

__global__ void k_sct_unpack(const u64* __restrict__ pair, int64_t n, int32_t* __restrict__ cid, int32_t* __restrict__ frag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cid[i] = (int32_t)(pair[i] >> 32);
    frag[i] = (int32_t)(uint32_t)pair[i];
}

__global__ void k_sct_sizes(const int32_t* __restrict__ owner, int64_t nel, int32_t n_clusters, int32_t* __restrict__ size)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nel) return;
    const int32_t o = owner[e];
    if (o >= 0 && o < n_clusters) atomicAdd(&size[o], 1);
}

// One lane per line (of either end): kept iff its cluster is one, kept at least min_size fragments and owns the line's
// fragment (tools/Parsers.cpp:146-159, with the lookups the reference leaves undefined passed over).  A fragment outside
// [0, max_element] and a cluster outside [0, n_clusters) are never looked up.
__global__ __launch_bounds__(BLOCK) void k_sct_keep(const PieceView* __restrict__ pv, int n_pieces, int64_t n_lines, int64_t n_out_lines,
                                                    const int32_t* __restrict__ cid, const int32_t* __restrict__ frag, const int32_t* __restrict__ owner,
                                                    const int32_t* __restrict__ size, int32_t n_clusters, int32_t max_element, int64_t min_size,
                                                    uint8_t* __restrict__ keep, uint32_t* __restrict__ klen, Summary* __restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<int, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool k = false;
    if (g < n_lines) {
        const int32_t c = cid[g], f = frag[g];
        k = g < n_out_lines && c >= 0 && c < n_clusters && (int64_t)size[c] >= min_size && f >= 0 && f <= max_element && owner[f] == c;
        uint32_t bytes = 0;
        if (k) {
            const PieceView P = pv[piece_of(pv, n_pieces, g)];
            const int64_t i = g - P.line_base;
            bytes = (uint32_t)(piece_line_end(P, i) - piece_line_start(P, i)) + 1u;        // the line and its newline, its own or the added one
        }
        keep[g] = k ? 1 : 0;
        klen[g] = bytes;
    }
    const int n = Reduce(tmp).Sum(k ? 1 : 0);
    if (threadIdx.x == 0 && n) atomicAdd(&sum->n_kept, (u64)n);
}

// the first line of a run: kept, and the line in front is not, or is in another piece, or the run has RUN_LINES lines
__global__ __launch_bounds__(BLOCK) void k_sct_heads(const PieceView* __restrict__ pv, int n_pieces, int64_t n_lines, const uint8_t* __restrict__ keep,
                                                     uint32_t* __restrict__ head)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_lines) return;
    uint32_t h = 0;
    if (keep[g]) {
        const int64_t i = g - pv[piece_of(pv, n_pieces, g)].line_base;
        h = (i == 0 || i % RUN_LINES == 0 || !keep[g - 1]) ? 1u : 0u;
    }
    head[g] = h;
}

// one thread, after the two exclusive sums
__global__ void k_sct_totals(int64_t n_lines, const uint32_t* __restrict__ klen, const u64* __restrict__ dst, const uint32_t* __restrict__ head,
                             const uint32_t* __restrict__ rank, Summary* __restrict__ sum)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    sum->out_bytes = (int64_t)(dst[n_lines - 1] + (u64)klen[n_lines - 1]);
    sum->n_runs = (int64_t)rank[n_lines - 1] + (int64_t)head[n_lines - 1];
}

// A head lane walks to the last line of its run (fewer than RUN_LINES steps) and writes the run's record.  A run that ends in
// its piece's last line where that has no newline copies up to the end of the text, and this lane stores the newline behind it.
__global__ __launch_bounds__(BLOCK) void k_sct_runs(const PieceView* __restrict__ pv, int n_pieces, int64_t n_lines, const uint8_t* __restrict__ keep,
                                                    const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, const u64* __restrict__ dst,
                                                    int64_t n_runs, Run* __restrict__ run, uint8_t* __restrict__ out, int64_t out_bytes,
                                                    Summary* __restrict__ sum)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_lines || !head[g] || (int64_t)rank[g] >= n_runs) return;
    const int p = piece_of(pv, n_pieces, g);
    const PieceView P = pv[p];
    const int64_t i = g - P.line_base;
    int64_t j = i;
    while (j + 1 < P.n_lines && (j + 1) % RUN_LINES != 0 && keep[P.line_base + j + 1]) ++j;
    const int64_t s0 = piece_line_start(P, i);
    const bool open_end = j >= P.n_nl;                                              // the piece's last line, without a newline
    const int64_t e1 = open_end ? P.len : (int64_t)P.nl_pos[j] + 1;
    const int64_t d = (int64_t)dst[g];
    run[rank[g]] = Run{s0, d, (uint32_t)(e1 - s0), (uint32_t)p};
    if (open_end && d + (e1 - s0) < out_bytes) {
        out[d + (e1 - s0)] = '\n';
        atomicAdd(&sum->n_added_nl, 1ull);
    }
}

// k_bat_gather of bat_shared.hpp without the reverse complement and with the source chosen per run: a group of G lanes owns a
// run and copies it by copy_span.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_sct_gather(const Run* __restrict__ run, int64_t n_runs, const PieceView* __restrict__ pv, int n_pieces,
                                                      uint8_t* __restrict__ dst, int64_t dst_len)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t k = t / G;
    const int lane = (int)(t % G);
    if (k >= n_runs) return;
    const Run r = run[k];
    if ((int64_t)r.piece >= (int64_t)n_pieces) return;
    const uint8_t* __restrict__ src = pv[r.piece].text;
    const int64_t src_len = pv[r.piece].len;
    const int64_t len = (int64_t)r.len;
    const int64_t d0 = r.dst;
    if (len == 0 || d0 < 0 || d0 + len > dst_len || r.src < 0 || r.src + len > src_len) return;
    (void)copy_span<G>(src, r.src, dst, d0, len, lane);
}

struct Piece {
    DeviceBuffer<uint8_t> text;
    DeviceBuffer<uint32_t> nl_pos;
    int64_t len = 0, n_nl = 0, n_lines = 0, line_base = 0, base = 0;
};

}  // namespace

struct sct_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[8];
    sct_timing timing{};
    std::vector<std::unique_ptr<Piece>> pieces;
    int64_t n_lines = 0, n_bytes = 0;
    TextScratch scratch;        // of a piece's tables
    // per line, over all pieces
    DeviceBuffer<PieceView, GrowSize> views;
    DeviceBuffer<int32_t, GrowSize> cid, frag;
    DeviceBuffer<uint8_t, GrowSize> meta, keep;
    DeviceBuffer<u64, GrowSize> dst;
    DeviceBuffer<uint32_t, GrowSize> klen, head, rank;
    DeviceBuffer<Summary> summary;
    // results of the last sct_cover
    DeviceBuffer<int32_t, GrowSize> owner;
    DeviceBuffer<uint8_t, GrowSize> out;
    int64_t out_bytes = 0, owner_n = 0;
    bool has_out = false;       // a cover has run on the pieces as they are: out[0, out_bytes) is its text
};

namespace {

// One piece into device memory (padded with zeros) with its newline table.  `len` > 0.
int add_piece(sct_ctx* c, const uint8_t* text, int64_t len)
{
    SCT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    std::unique_ptr<Piece> pc(new Piece());
    SCT_HIP(pc->text.reserve(padded_size(len)));
    Totals tot{};
    if (const int rc = text_upload_count<false>(g_sct_err, c->scratch, pc->text.p, text, hipMemcpyHostToDevice, len, c->ev[0], c->ev[1], st, tot)) return rc;
    const int64_t n_nl = (int64_t)tot.n_nl;
    const int64_t n_lines = n_nl + (tot.last != '\n' ? 1 : 0);
    if (c->n_lines + n_lines > (int64_t)INT32_MAX) return SCT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 cluster lines");
    SCT_HIP(pc->nl_pos.reserve((size_t)n_nl));
    text_place_tables<false>(c->scratch, pc->text.p, len, tot, pc->nl_pos.p, nullptr, nullptr, st);
    SCT_HIP(hipEventRecord(c->ev[2], st));
    SCT_HIP(hipStreamSynchronize(st));
    SCT_HIP(hipGetLastError());
    pc->len = len;
    pc->n_nl = n_nl;
    pc->n_lines = n_lines;
    pc->line_base = c->n_lines;
    pc->base = c->n_bytes;
    c->n_lines += n_lines;
    c->n_bytes += len;
    c->pieces.push_back(std::move(pc));
    c->timing.upload_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.tables_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.text_bytes = c->n_bytes;
    c->timing.n_pieces = (int32_t)c->pieces.size();
    return DSA_OK;
}

int bits_for(int64_t max_value)
{
    int bits = 1;
    while ((1ll << bits) <= max_value) ++bits;
    return bits;
}

int cover_run(sct_ctx* c, int64_t min_size, sct_result* r)
{
    SCT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t n = c->n_lines;
    const int np = (int)c->pieces.size();
    r->n_lines = n;
    r->max_element = -1;
    if (n == 0) return DSA_OK;

    std::vector<PieceView> views;
    for (const auto& pc : c->pieces) views.push_back(PieceView{pc->text.p, pc->nl_pos.p, pc->len, pc->n_nl, pc->n_lines, pc->line_base, pc->base});
    SCT_HIP(c->views.reserve(views.size()));
    SCT_HIP(c->cid.reserve((size_t)n));
    SCT_HIP(c->frag.reserve((size_t)n));
    SCT_HIP(c->meta.reserve((size_t)n));
    SCT_HIP(c->keep.reserve((size_t)n));
    SCT_HIP(c->summary.reserve(1));
    Summary sum{};
    sum.rstop = sum.wstop = NONE;
    sum.max_cid = sum.max_el = -1;
    SCT_HIP(hipMemcpyAsync(c->views.p, views.data(), views.size() * sizeof(PieceView), hipMemcpyHostToDevice, st));
    SCT_HIP(hipMemcpyAsync(c->summary.p, &sum, sizeof(Summary), hipMemcpyHostToDevice, st));
    const PieceView* pv = c->views.p;
    const unsigned gl = grid_of(n);

    // parse (the member flags go where the keep flags go later)
    SCT_HIP(hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_sct_lines, dim3(gl), dim3(BLOCK), 0, st, pv, np, n, c->cid.p, c->frag.p, c->meta.p, c->keep.p, c->summary.p);
    SCT_HIP(hipEventRecord(c->ev[1], st));
    SCT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
    SCT_HIP(hipStreamSynchronize(st));
    SCT_HIP(hipGetLastError());
    c->timing.parse_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    const bool read_stop = (int64_t)sum.rstop < n, write_stop = !read_stop && (int64_t)sum.wstop < n;
    if (sum.n_members > (u64)n || sum.max_cid < -1 || sum.max_el < -1)
        return SCT_FAIL(DSA_E_DEVICE, "internal: %llu end-0 lines of %lld", sum.n_members, (long long)n);
    if (read_stop || write_stop) {
        const int64_t g = read_stop ? (int64_t)sum.rstop : (int64_t)sum.wstop;
        hipLaunchKernelGGL(k_sct_stop, dim3(1), dim3(64), 0, st, pv, np, g, (const uint8_t*)c->meta.p, write_stop ? 1 : 0, c->summary.p);
        SCT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
        SCT_HIP(hipStreamSynchronize(st));
        SCT_HIP(hipGetLastError());
        r->stop_kind = (int32_t)sum.stop_kind;
        r->stop_line = g + 1;
        r->stop_offset = sum.stop_offset;
        r->stop_len = sum.stop_len;
    }
    if (read_stop) { r->status = SCT_READ_STOP; return DSA_OK; }
    r->n_members = (int64_t)sum.n_members;
    r->n_clusters = (int64_t)sum.max_cid + 1;
    r->max_element = sum.max_el;
    if (sum.negative) {
        r->status = SCT_NEGATIVE_ELEMENT;
        r->stop_kind = 0;
        r->stop_line = r->stop_offset = r->stop_len = 0;
        return DSA_OK;
    }
    r->status = write_stop ? SCT_WRITE_STOP : SCT_OK;
    const int64_t n_members = (int64_t)sum.n_members;
    if (n_members == 0) return DSA_OK;                          // no cluster: nothing is kept
    if (sum.max_cid == INT32_MAX || sum.max_el == INT32_MAX)
        return SCT_FAIL(DSA_E_LIMIT, "a cluster id or fragment of 2^31 - 1 on an end-0 line: the tables would have 2^31 entries");
    const int32_t n_clusters = sum.max_cid + 1, max_element = sum.max_el;
    const int64_t nel = (int64_t)max_element + 1;

    // layout: clusters[id] = the end-0 lines' fragments in file order
    DeviceBuffer<int64_t> d_coff;
    DeviceBuffer<int32_t> d_el, d_size;
    {
        DeviceBuffer<u64> m_pair, s_pair;                       // (cluster << 32 | fragment) of the end-0 lines
        DeviceBuffer<int32_t> s_cid, d_count;
        SCT_HIP(m_pair.reserve((size_t)n_members));
        SCT_HIP(s_pair.reserve((size_t)n_members));
        SCT_HIP(s_cid.reserve((size_t)n_members));
        SCT_HIP(d_el.reserve((size_t)n_members));
        SCT_HIP(d_count.reserve(1));
        SCT_HIP(d_coff.reserve((size_t)n_clusters + 1));
        hipcub::TransformInputIterator<u64, PackMember, hipcub::CountingInputIterator<int64_t>> pairs(hipcub::CountingInputIterator<int64_t>(0),
                                                                                                      PackMember{c->cid.p, c->frag.p});
        SCT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceSelect::Flagged(w, wb, pairs, c->keep.p, m_pair.p, d_count.p, (int)n, st);
        }));
        SCT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {         // stable, by the cluster half only: file order inside a cluster
            return hipcub::DeviceRadixSort::SortKeys(w, wb, m_pair.p, s_pair.p, (int)n_members, 32, 32 + bits_for(sum.max_cid), st);
        }));
        hipLaunchKernelGGL(k_sct_unpack, dim3(grid_of(n_members)), dim3(BLOCK), 0, st, (const u64*)s_pair.p, n_members, s_cid.p, d_el.p);
        hipLaunchKernelGGL(k_lower_bounds, dim3(grid_of((int64_t)n_clusters + 1)), dim3(BLOCK), 0, st, (const int32_t*)s_cid.p, n_members, n_clusters - 1,
                           d_coff.p);
        SCT_HIP(hipEventRecord(c->ev[2], st));
    }                                                           // (freeing the temporaries waits for what reads them)

    // cover
    SCT_HIP(c->owner.reserve((size_t)nel));
    sc_timing sc_t{};
    if (const int rc = sc_cover_device(g_sct_err, st, d_coff.p, d_el.p, n_clusters, n_members, max_element, c->owner.p, sc_t)) return rc;
    c->owner_n = nel;
    c->timing.layout_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.cover_ms = sc_t.total_ms;
    c->timing.n_components = sc_t.n_components;
    c->timing.n_large = sc_t.n_large;
    c->timing.cc_iterations = sc_t.cc_iterations;

    // select
    SCT_HIP(d_size.reserve((size_t)n_clusters));
    SCT_HIP(c->klen.reserve((size_t)n));
    SCT_HIP(c->dst.reserve((size_t)n));
    SCT_HIP(c->head.reserve((size_t)n));
    SCT_HIP(c->rank.reserve((size_t)n));
    SCT_HIP(hipEventRecord(c->ev[3], st));
    SCT_HIP(hipMemsetAsync(d_size.p, 0, (size_t)n_clusters * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_sct_sizes, dim3(grid_of(nel)), dim3(BLOCK), 0, st, (const int32_t*)c->owner.p, nel, n_clusters, d_size.p);
    const int64_t n_out_lines = write_stop ? (int64_t)sum.wstop : n;
    hipLaunchKernelGGL(k_sct_keep, dim3(gl), dim3(BLOCK), 0, st, pv, np, n, n_out_lines, (const int32_t*)c->cid.p, (const int32_t*)c->frag.p,
                       (const int32_t*)c->owner.p, (const int32_t*)d_size.p, n_clusters, max_element, min_size, c->keep.p, c->klen.p, c->summary.p);
    hipLaunchKernelGGL(k_sct_heads, dim3(gl), dim3(BLOCK), 0, st, pv, np, n, (const uint8_t*)c->keep.p, c->head.p);
    hipcub::TransformInputIterator<u64, Widen, const uint32_t*> lengths(c->klen.p, Widen());      // 32-bit lengths, a 64-bit sum
    SCT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, lengths, c->dst.p, (int)n, st); }));
    SCT_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->head.p, c->rank.p, (int)n, st); }));
    hipLaunchKernelGGL(k_sct_totals, dim3(1), dim3(64), 0, st, n, (const uint32_t*)c->klen.p, (const u64*)c->dst.p, (const uint32_t*)c->head.p,
                       (const uint32_t*)c->rank.p, c->summary.p);
    SCT_HIP(hipEventRecord(c->ev[4], st));
    SCT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
    SCT_HIP(hipStreamSynchronize(st));
    SCT_HIP(hipGetLastError());
    c->timing.select_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    if (sum.out_bytes < 0 || sum.out_bytes > c->n_bytes + (int64_t)np || sum.n_runs < 0 || sum.n_runs > n || sum.n_kept > (u64)n)
        return SCT_FAIL(DSA_E_DEVICE, "internal: %lld output bytes in %lld runs of %lld input bytes", (long long)sum.out_bytes, (long long)sum.n_runs,
                        (long long)c->n_bytes);
    r->n_kept_lines = (int64_t)sum.n_kept;

    // gather
    if (sum.n_runs) {
        DeviceBuffer<Run> runs;
        SCT_HIP(runs.reserve((size_t)sum.n_runs));
        SCT_HIP(c->out.reserve((size_t)sum.out_bytes + 8));     // whole dwords
        hipLaunchKernelGGL(k_sct_runs, dim3(gl), dim3(BLOCK), 0, st, pv, np, n, (const uint8_t*)c->keep.p, (const uint32_t*)c->head.p,
                           (const uint32_t*)c->rank.p, (const u64*)c->dst.p, sum.n_runs, runs.p, c->out.p, sum.out_bytes, c->summary.p);
        hipLaunchKernelGGL(k_sct_gather<RUN_GROUP>, dim3(grid_of(sum.n_runs * RUN_GROUP)), dim3(BLOCK), 0, st, (const Run*)runs.p, sum.n_runs, pv, np, c->out.p,
                           sum.out_bytes);
        SCT_HIP(hipEventRecord(c->ev[5], st));
        SCT_HIP(hipMemcpyAsync(&sum, c->summary.p, sizeof(Summary), hipMemcpyDeviceToHost, st));
        SCT_HIP(hipStreamSynchronize(st));
        SCT_HIP(hipGetLastError());
        c->timing.gather_ms = hiphost::elapsed(c->ev[4], c->ev[5]);
    }
    c->out_bytes = r->out_bytes = sum.out_bytes;
    c->timing.gather_bytes = sum.out_bytes - (int64_t)sum.n_added_nl;
    c->timing.n_runs = sum.n_runs;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* sct_last_error(void) { return g_sct_err.c_str(); }

int sct_create(int device, sct_ctx** out)
{
    if (!out) return SCT_FAIL(DSA_E_ARG, "sct_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_sct_err)) return DSA_E_DEVICE;
    SCT_HIP(hipSetDevice(device));
    sct_ctx* c = new sct_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return SCT_FAIL(DSA_E_DEVICE, "cannot create a stream or an event");
    }
    *out = c;
    return DSA_OK;
}

void sct_destroy(sct_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int sct_begin(sct_ctx* c)
{
    if (!c) return SCT_FAIL(DSA_E_ARG, "sct_begin: no ctx");
    SCT_HIP(hipSetDevice(c->device));
    SCT_HIP(hipStreamSynchronize(c->st));
    c->pieces.clear();
    c->n_lines = c->n_bytes = 0;
    c->out_bytes = c->owner_n = 0;
    c->has_out = false;
    c->timing = sct_timing{};
    return DSA_OK;
}

int sct_add(sct_ctx* c, const uint8_t* text, int64_t len, int32_t final, int64_t* consumed)
{
    if (!consumed) return SCT_FAIL(DSA_E_ARG, "sct_add: no place for the consumed count");
    *consumed = 0;
    if (len < 0) return SCT_FAIL(DSA_E_ARG, "sct_add: negative length (%lld)", (long long)len);
    if (len > (int64_t)INT32_MAX) return SCT_FAIL(DSA_E_LIMIT, "sct_add: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", (long long)len);
    if (len && !text) return SCT_FAIL(DSA_E_ARG, "sct_add: null pointer with non-zero size");
    if (final != 0 && final != 1) return SCT_FAIL(DSA_E_ARG, "sct_add: final %d is not 0 or 1", final);
    if (!c) return SCT_FAIL(DSA_E_ARG, "sct_add: no ctx");
    if (!final) len = whole_lines(text, len);
    if (len == 0) return DSA_OK;
    c->out_bytes = c->owner_n = 0;                              // the last cover's results are of another input
    c->has_out = false;
    const int rc = add_piece(c, text, len);
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);        // nothing of a refused call is in flight when it returns
    else *consumed = len;
    return rc;
}

int sct_cover(sct_ctx* c, int64_t min_cluster_size, sct_result* r)
{
    if (!r) return SCT_FAIL(DSA_E_ARG, "sct_cover: no result");
    *r = sct_result{};
    if (!c) return SCT_FAIL(DSA_E_ARG, "sct_cover: no ctx");
    c->out_bytes = c->owner_n = 0;
    c->has_out = false;
    c->timing.parse_ms = c->timing.layout_ms = c->timing.cover_ms = c->timing.select_ms = c->timing.gather_ms = c->timing.download_ms = 0.f;
    c->timing.gather_bytes = c->timing.n_runs = 0;
    c->timing.n_components = c->timing.n_large = c->timing.cc_iterations = 0;
    const int rc = cover_run(c, min_cluster_size, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->out_bytes = c->owner_n = 0;
        *r = sct_result{};
    } else c->has_out = r->status == SCT_OK || r->status == SCT_WRITE_STOP;
    return rc;
}

int sct_fetch(sct_ctx* c, int64_t offset, uint8_t* buf, int64_t len)
{
    if (!c) return SCT_FAIL(DSA_E_ARG, "sct_fetch: no ctx");
    if (offset < 0 || len < 0 || offset > c->out_bytes || len > c->out_bytes - offset)
        return SCT_FAIL(DSA_E_ARG, "sct_fetch: [%lld, +%lld) is outside the %lld output bytes", (long long)offset, (long long)len, (long long)c->out_bytes);
    if (len && !buf) return SCT_FAIL(DSA_E_ARG, "sct_fetch: length without a buffer");
    if (len == 0) return DSA_OK;
    SCT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    SCT_HIP(hipEventRecord(c->ev[6], st));
    SCT_HIP(hipMemcpyAsync(buf, c->out.p + offset, (size_t)len, hipMemcpyDeviceToHost, st));
    SCT_HIP(hipEventRecord(c->ev[7], st));
    SCT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms += hiphost::elapsed(c->ev[6], c->ev[7]);
    return DSA_OK;
}

int sct_fetch_owner(sct_ctx* c, int32_t* owner, int64_t cap)
{
    if (!c) return SCT_FAIL(DSA_E_ARG, "sct_fetch_owner: no ctx");
    if (cap < 0 || (cap && !owner)) return SCT_FAIL(DSA_E_ARG, "sct_fetch_owner: %s", cap < 0 ? "negative capacity" : "capacity without a buffer");
    if (cap < c->owner_n) return SCT_FAIL(DSA_E_CAPACITY, "the set cover has %lld fragments", (long long)c->owner_n);
    if (c->owner_n == 0) return DSA_OK;
    SCT_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    SCT_HIP(hipEventRecord(c->ev[6], st));
    SCT_HIP(hipMemcpyAsync(owner, c->owner.p, (size_t)c->owner_n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SCT_HIP(hipEventRecord(c->ev[7], st));
    SCT_HIP(hipStreamSynchronize(st));
    c->timing.download_ms += hiphost::elapsed(c->ev[6], c->ev[7]);
    return DSA_OK;
}

int sct_get_timing(const sct_ctx* c, sct_timing* out)
{
    if (!c || !out) return SCT_FAIL(DSA_E_ARG, "sct_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"

// taskc_api.hip: where the last cover's output lies (no public header has this).  False if there is none.
__attribute__((visibility("hidden"))) bool sct_cover_output_device(const sct_ctx* c, int* device, const uint8_t** text, int64_t* len)
{
    if (!c || !c->has_out) return false;
    *device = c->device;
    *text = c->out.p;
    *len = c->out_bytes;
    return true;
}
