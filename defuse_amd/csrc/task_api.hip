// task_api.hip — CreateTasks / SplitAlignmentTask::Initialize (tools/SplitAlignment.cpp:31-175, 637-685) for all fusions of
// a run on gfx950 (include/defuse_task.h): the windows, remainders and mate regions of every task, made on the device from
// the integers of the regions file, a reference kept in device memory and the exon table.
//
// task_store_create, all on one stream, one host round trip:
//   (1) plan: one thread per (task, end) computes the break region, the two clipped cuts of FastaIndex::Get, the walk from the
//       transcript to the genome, mateMin / mateMax, the genomic mate region and the end's status bits;
//   (2) count: a group of REGION_GROUP lanes per (task, end) walks the bin of its mate region; every lane tests one transcript
//       (overlap, RemapThroughTranscript) and a ballot counts the regions;
//   (3) three 64-bit exclusive sums (window bytes, remainder bytes, regions); the totals and the lowest task with a window
//       beyond the DP's limit come back in one small copy and are tested before the pools are sized;
//   (4) emit: the kernel of (2) again, now writing; the ballot's prefix keeps a bin's ascending transcript order without a
//       sort.  A mate region that touches several bins (rare: it is a few hundred bases, a bin 100000) takes the transcripts of
//       its bins in ascending order through repeated lower bounds, all lanes alike, which is the same order;
//   (5) records and one segment descriptor per window and per remainder, then the gather (k_bat_gather of bat_shared.hpp):
//       windows through Seg, remainders through Seg64;
//   (6) a radix sort of (fusion_id, task) gives the key order of bat_windows and pred_tasks, which one kernel fills.
// Every byte of the pools has one writer, a segment's group; every region one, a lane of its end's group.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <string>

#include "../../include/defuse_task.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "pred_shared.hpp"
#include "task_check.hpp"

namespace {

using batdev::Seg;
using batdev::Seg64;
using batdev::SRC_PAD;
using hiphost::DeviceBuffer;
using hiphost::grid_of;
using predint::DevTask;
using u64 = unsigned long long;

thread_local std::string g_task_err;

#define TASK_HIP(call) HIPHOST_TRY(g_task_err, call)
#define TASK_FAIL(code, ...) hiphost::fail(g_task_err, code, __VA_ARGS__)

constexpr int BLOCK = batdev::GATHER_BLOCK;
constexpr int REGION_GROUP = 16;      // lanes per (task, end): a bin of 100000 bases holds a handful of transcripts
constexpr int REM_GROUP = 16;         // lanes per remainder: none to a few hundred bases
constexpr int WINDOW_GROUP = 64;      // lanes per window: a few hundred bases and more
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int PLUS = 0, MINUS = 1;

static_assert(sizeof(task_seq) == 16 && sizeof(task_transcript) == 20 && sizeof(task_exon) == 8 && sizeof(task_params) == 16 && sizeof(task_end) == 24 &&
                  sizeof(task_pair) == 52 && sizeof(task_record) == 80 && sizeof(task_counts) == 32 && sizeof(task_timing) == 64,
              "C ABI layout");
static_assert(BLOCK % 64 == 0 && 64 % REGION_GROUP == 0, "a group lies in one wave");

struct ExonsView {
    const task_transcript* tx;
    const int32_t* tx_len;
    const int2* tx_reg;
    const task_exon* exons;
    const int32_t* chrom_ref;
    const int32_t* chrom_bin_lo;
    const int32_t* chrom_bins;
    const int32_t* chrom_row;
    const int32_t* row_first;
    const int32_t* row_tx;
};

// what the plan leaves of a (task, end) for the kernels after it
struct EndPlan {
    int64_t win_src, rem_src;   // offsets into the reference bytes
    int32_t win_len, rem_len;   // bytes cut
    int32_t seq_start, seq_len; // start and length as Get left them
    int32_t seq_strand;
    int32_t status;             // TASK_* bits of this end
    int32_t chrom;              // of the genomic mate region, -1 with TASK_BAD_CHROMOSOME_*
    int32_t gstrand, gbreak;    // genomeAlignStrand, genomeBreakRegionStart
    int32_t q0, q1;             // genomeMateRegion
    int32_t mate_min, mate_max;
    int32_t pad_;
};

struct Totals {
    uint32_t long_window;       // lowest task with a window beyond the DP's limit, NONE if there is none
    uint32_t pad_;
};

struct Cut {
    int64_t src;
    int32_t len;
    int32_t start, length;      // the int& parameters on return
    bool missing;
};

// FastaIndex::Get (tools/FastaIndex.cpp:23-61, faidx.c:305-357) without the bytes
__device__ inline Cut fasta_get(const task_seq* __restrict__ seqs, int32_t seq, int32_t start, int32_t length)
{
    if (length < 0) return Cut{0, 0, start, length, false};
    if (start < 1) {
        length -= 1 - start;
        start = 1;
    }
    const int32_t end = start + length - 1;
    if (seq < 0) return Cut{0, 0, start, length, true};
    const task_seq s = seqs[seq];
    const int32_t L = (int32_t)s.len;
    int32_t beg = start - 1, e = end;
    if (beg >= L) beg = L;
    if (e < 0 || e >= L) e = L;           // (faidx compares with an unsigned field: a negative end is beyond the sequence)
    if (beg > e) beg = e;
    return Cut{s.off + beg, e - beg, start, e - beg, false};
}

__global__ __launch_bounds__(BLOCK) void k_task_plan(const task_pair* __restrict__ pairs, int64_t n_ends, task_params P, const task_seq* __restrict__ seqs,
                                                      ExonsView X, int32_t max_window, EndPlan* __restrict__ plan, u64* __restrict__ wlen,
                                                      u64* __restrict__ rlen, Totals* __restrict__ tot)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_ends) return;
    const int ce = (int)(i & 1);
    const task_end a = pairs[i >> 1].end[ce];
    // CalculateBreakRegion (tools/SplitAlignment.cpp:637-655)
    const int32_t region_len = a.end - a.start + 1;
    const int32_t push = min(P.max_read, region_len / 2);                 // (int)(0.5 * regionLength): toward zero
    const int32_t blen = P.max_fragment - region_len - P.min_read + 2 * push;
    const int32_t bstart = a.strand == PLUS ? a.end - push + 1 : a.start + push - 1;
    EndPlan p{};
    p.seq_strand = ce == 0 ? a.strand : 1 - a.strand;
    const Cut w = fasta_get(seqs, a.seq, a.strand == PLUS ? bstart - P.max_read : bstart - blen + 1, blen + P.max_read);
    p.seq_start = w.start;
    p.seq_len = w.length;
    p.win_src = w.src;
    p.win_len = w.len;
    bool missing = w.missing;
    Cut r{0, 0, 0, 0, false};
    if (a.strand == PLUS) {
        if (a.start < w.start) r = fasta_get(seqs, a.seq, a.start, w.start - 1 - a.start + 1);
    } else if (a.end > w.start + w.length - 1) {
        const int32_t rs = w.start + w.length;
        r = fasta_get(seqs, a.seq, rs, a.end - rs + 1);
    }
    missing = missing || r.missing;
    p.rem_src = r.src;
    p.rem_len = r.len;
    if (p.win_len > max_window) {
        atomicMin(&tot->long_window, (uint32_t)(i >> 1));
        p.win_len = 0;
    }
    // RemapTranscriptToGenome (tools/ExonRegions.cpp:258-302) or the name itself
    p.chrom = a.chrom;
    p.gstrand = a.strand;
    p.gbreak = bstart;
    if (a.transcript >= 0) {
        const task_transcript t = X.tx[a.transcript];
        const int32_t tlen = X.tx_len[a.transcript];
        const int32_t pos = t.strand == MINUS ? tlen - bstart + 1 : bstart;
        p.chrom = t.chrom;
        p.gstrand = t.strand == a.strand ? PLUS : MINUS;
        p.gbreak = pos - tlen + X.exons[t.first_exon + t.n_exons - 1].end;
        int32_t off = 0;
        for (int32_t k = 0; k < t.n_exons; ++k) {
            const task_exon e = X.exons[t.first_exon + k];
            const int32_t len = e.end - e.start + 1;
            if (pos <= off + len) {
                p.gbreak = pos - (off + 1) + e.start;
                break;
            }
            off += len;
        }
    }
    const bool bad_chrom = p.chrom < 0 || X.chrom_bins[p.chrom] == 0;
    if (bad_chrom) p.chrom = -1;
    p.mate_min = P.min_fragment - blen - P.max_read + 1;
    p.mate_max = P.max_fragment - P.min_read;
    p.q0 = p.gstrand == PLUS ? p.gbreak - p.mate_max : p.gbreak + p.mate_min;
    p.q1 = p.gstrand == PLUS ? p.gbreak - p.mate_min : p.gbreak + p.mate_max;
    p.status = ((missing ? TASK_NO_SEQUENCE_0 : 0) | (bad_chrom ? TASK_BAD_CHROMOSOME_0 : 0)) << (2 * ce);
    plan[i] = p;
    wlen[i] = (u64)p.win_len;
    rlen[i] = (u64)p.rem_len;
}

// RemapThroughTranscript (tools/ExonRegions.cpp:421-482) of a position on `strand`; the exons of the minus strand are the
// negated ones in reverse order (TransformExons, :114-124)
__device__ inline bool remap_through(const ExonsView& X, int32_t t, int32_t position, int32_t strand, int32_t ext_min, int32_t ext_max, cand_region* out)
{
    const task_transcript x = X.tx[t];
    const int32_t tlen = X.tx_len[t];
    const task_exon* __restrict__ ex = X.exons + x.first_exon;
    const int32_t sp = strand == PLUS ? position : -position;
    if (sp > (strand == PLUS ? ex[x.n_exons - 1].end : -ex[0].start)) return false;
    int32_t off = 0, start = 0, end = 0;
    for (int32_t k = 0; k < x.n_exons; ++k) {
        const task_exon g = ex[strand == PLUS ? k : x.n_exons - 1 - k];
        const int32_t b = strand == PLUS ? g.start : -g.end, e = strand == PLUS ? g.end : -g.start;
        if (sp <= e) {
            const int32_t rs = sp - b + ext_min + 1, re = sp - b + ext_max + 1;
            if (re < 1) return false;
            start = max(1, rs) + off;
            end = max(1, re) + off;
            break;
        }
        off += e - b + 1;
    }
    if (end < 1 || start > tlen) return false;
    if (strand != x.strand) {
        const int32_t s = tlen - end + 1;
        end = tlen - start + 1;
        start = s;
    }
    out->ref = x.name_ref;
    out->strand = 1 - (strand == x.strand ? PLUS : MINUS);      // (tools/SplitAlignment.cpp:163)
    out->start = start;
    out->end = end;
    return true;
}

// the first index in [lo, hi) with a[index] >= x
__device__ inline int32_t lower_bound(const int32_t* __restrict__ a, int32_t lo, int32_t hi, int32_t x)
{
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// GetRegionTranscripts (tools/ExonRegions.cpp:131-161) and the loop over its result (tools/SplitAlignment.cpp:147-171) of one
// (task, end) per group.  EMIT false: count[i] = its regions; EMIT true: they are written at off[i].
template <bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_task_regions(const EndPlan* __restrict__ plan, int64_t n_ends, ExonsView X, const task_pair* __restrict__ pairs,
                                                         u64* __restrict__ count, const u64* __restrict__ off, cand_region* __restrict__ out, int64_t n_out)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i = t / REGION_GROUP;
    const int lane = (int)(t % REGION_GROUP);
    if (i >= n_ends) return;
    const EndPlan p = plan[i];
    if (p.chrom < 0) {
        if (!EMIT && lane == 0) count[i] = 0;
        return;
    }
    const int shift = (int)(threadIdx.x & 63) / REGION_GROUP * REGION_GROUP;
    const int32_t id = (int32_t)(((uint32_t)pairs[i >> 1].fusion_id & 0x7FFFFFFFu) | ((uint32_t)(i & 1) << 31));
    const int64_t base = EMIT ? (int64_t)off[i] : 0;
    int64_t pos = 1;                                                        // after the genomic region
    auto put = [&](int64_t at, cand_region r) {
        r.id = id;
        if (base + at >= 0 && base + at < n_out) out[base + at] = r;
    };
    if (EMIT && lane == 0) put(0, cand_region{X.chrom_ref[p.chrom], p.gstrand, p.q0, p.q1, id});
    const int32_t lo = X.chrom_bin_lo[p.chrom], row0 = X.chrom_row[p.chrom];
    const int32_t qb0 = p.q0 / TASK_EXON_BIN, qb1 = p.q1 / TASK_EXON_BIN;
    const int32_t b0 = max(qb0, lo), b1 = min(qb1, lo + X.chrom_bins[p.chrom] - 1);
    auto overlaps = [&](int32_t tr) {
        const int2 r = X.tx_reg[tr];
        return !(r.y < p.q0 || r.x > p.q1);
    };
    if (b0 == b1) {
        // one bin: its transcripts are ascending, a lane each
        const int32_t first = X.row_first[row0 + (b0 - lo)], last = X.row_first[row0 + (b0 - lo) + 1];
        for (int32_t j0 = first; j0 < last; j0 += REGION_GROUP) {
            const int32_t j = j0 + lane;
            cand_region r{};
            const bool ok = j < last && overlaps(X.row_tx[j]) && remap_through(X, X.row_tx[j], p.gbreak, 1 - p.gstrand, p.mate_min, p.mate_max, &r);
            const uint32_t mask = (uint32_t)(__ballot(ok) >> shift) & ((1u << REGION_GROUP) - 1u);
            if (EMIT && ok) put(pos + __popc(mask & ((1u << lane) - 1u)), r);
            pos += __popc(mask);
        }
    } else if (b0 < b1) {
        // several bins: the smallest transcript above the last one taken, over all bins; every lane walks alike
        int32_t next = 0;
        while (true) {
            int32_t best = INT32_MAX;
            for (int32_t b = b0; b <= b1; ++b) {
                const int32_t first = X.row_first[row0 + (b - lo)], last = X.row_first[row0 + (b - lo) + 1];
                const int32_t j = lower_bound(X.row_tx, first, last, next);
                if (j < last) best = min(best, X.row_tx[j]);
            }
            if (best == INT32_MAX) break;
            next = best + 1;
            cand_region r{};
            if (overlaps(best) && remap_through(X, best, p.gbreak, 1 - p.gstrand, p.mate_min, p.mate_max, &r)) {
                if (EMIT && lane == 0) put(pos, r);
                ++pos;
            }
        }
    }
    if (!EMIT && lane == 0) count[i] = (u64)pos;
}

// the record of every task, and one gather segment per window and per remainder
__global__ __launch_bounds__(BLOCK) void k_task_records(const task_pair* __restrict__ pairs, int64_t n, const EndPlan* __restrict__ plan,
                                                         const u64* __restrict__ woff, const u64* __restrict__ roff, const u64* __restrict__ goff,
                                                         const u64* __restrict__ gcount, task_record* __restrict__ rec, uint32_t* __restrict__ key,
                                                         uint32_t* __restrict__ idx, Seg* __restrict__ seg_win, Seg64* __restrict__ seg_rem)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    task_record r{};
    r.fusion_id = pairs[k].fusion_id;
    r.region_off = (int64_t)goff[2 * k];
    for (int e = 0; e < 2; ++e) {
        const EndPlan p = plan[2 * k + e];
        r.status |= p.status;
        r.seq_start[e] = p.seq_start;
        r.seq_len[e] = p.seq_len;
        r.seq_strand[e] = p.seq_strand;
        r.win_off[e] = (int32_t)woff[2 * k + e];                            // (the total has been tested)
        r.rem_len[e] = p.rem_len;
        r.rem_off[e] = (int64_t)roff[2 * k + e];
        r.n_regions[e] = (int32_t)gcount[2 * k + e];
        const uint32_t rev = p.seq_strand == MINUS ? 0x80000000u : 0u;
        seg_win[2 * k + e] = Seg{p.win_src, r.win_off[e], (uint32_t)p.win_len | rev};
        seg_rem[2 * k + e] = Seg64{p.rem_src, r.rem_off[e], (uint32_t)p.rem_len | rev, 0};
    }
    rec[k] = r;
    key[k] = (uint32_t)r.fusion_id;
    idx[k] = (uint32_t)k;
}

// bat_windows and pred_tasks in key order
__global__ __launch_bounds__(BLOCK) void k_task_stores(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx, int64_t n,
                                                        const task_record* __restrict__ rec, const EndPlan* __restrict__ plan, uint32_t* __restrict__ wkey,
                                                        dsa_fusion* __restrict__ wfus, uint32_t* __restrict__ tkey, DevTask* __restrict__ task)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n || (int64_t)idx[s] >= n) return;
    const int64_t k = idx[s];
    const task_record r = rec[k];
    wkey[s] = tkey[s] = key[s];
    wfus[s] = dsa_fusion{r.fusion_id, r.win_off[0], plan[2 * k].win_len, r.win_off[1], plan[2 * k + 1].win_len};
    task[s] = DevTask{{r.rem_off[0], r.rem_off[1]}, {r.rem_len[0], r.rem_len[1]}, {r.win_off[0], r.win_off[1]}, {r.seq_start[0], r.seq_start[1]},
                      {r.seq_len[0], r.seq_len[1]}, {r.seq_strand[0], r.seq_strand[1]}, {0, 0}};
}

template <class T>
int upload(DeviceBuffer<T>& buf, const T* host, size_t n, hipStream_t st)
{
    TASK_HIP(buf.reserve(n));
    if (n) TASK_HIP(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, st));
    return DSA_OK;
}

}  // namespace

struct __attribute__((visibility("hidden"))) task_reference {
    int device = -1;
    int64_t n_seqs = 0, bytes_len = 0;
    DeviceBuffer<uint8_t> bytes;            // bytes_len + SRC_PAD
    DeviceBuffer<task_seq> seqs;
};

struct __attribute__((visibility("hidden"))) task_exons {
    int device = -1;
    int32_t n_chroms = 0, n_tx = 0;
    DeviceBuffer<task_transcript> tx;
    DeviceBuffer<int32_t> tx_len, tx_reg, chrom_ref, chrom_bin_lo, chrom_bins, chrom_row, row_first, row_tx;
    DeviceBuffer<task_exon> exons;
    ExonsView view() const
    {
        return ExonsView{tx.p, tx_len.p, reinterpret_cast<const int2*>(tx_reg.p), exons.p, chrom_ref.p, chrom_bin_lo.p, chrom_bins.p, chrom_row.p, row_first.p,
                         row_tx.p};
    }
};

struct __attribute__((visibility("hidden"))) task_store {
    int device = -1;
    int64_t n = 0, n_regions = 0;
    hiphost::Stream st;
    hiphost::Event ev[10];      // 0 start, 1 uploaded, 2 planned, 3 counted, 4 summed, 5 emitted and described, 6 gathered, 7 sorted; 8, 9 around a fetch
    bat_windows windows;
    pred_tasks tasks;
    DeviceBuffer<task_record> records;
    DeviceBuffer<cand_region> regions;
    task_timing timing{};
};

namespace {

int open_store(task_store* s)
{
    if (s->st.create(hipStreamNonBlocking) != hipSuccess) return TASK_FAIL(DSA_E_DEVICE, "cannot create a stream");
    for (auto& e : s->ev)
        if (e.create() != hipSuccess) return TASK_FAIL(DSA_E_DEVICE, "cannot create an event");
    return DSA_OK;
}

// Everything of task_store_create on the device, behind the upload: `pairs` are n pairs in device memory, which the store's
// stream may read (the caller has recorded ev[0] and ev[1] around whatever brought them there, if n > 0).
int build_store(task_store* s, const task_reference* ref, const task_exons* ex, const task_params& P, const task_pair* pairs, int64_t n)
{
    hipStream_t st = s->st;
    const int64_t E = 2 * n;
    // the stores have pointers, whatever n
    TASK_HIP(s->records.reserve((size_t)n));
    TASK_HIP(s->windows.wkey.reserve((size_t)n));
    TASK_HIP(s->windows.wfus.reserve((size_t)n));
    TASK_HIP(s->tasks.tkey.reserve((size_t)n));
    TASK_HIP(s->tasks.task.reserve((size_t)n));
    s->windows.device = s->tasks.device = s->device;
    s->windows.n = s->tasks.n = n;
    s->tasks.windows = &s->windows;
    if (n == 0) {
        TASK_HIP(s->windows.bytes.reserve(SRC_PAD));
        TASK_HIP(s->tasks.rem.reserve(SRC_PAD));
        TASK_HIP(s->regions.reserve(1));
        return DSA_OK;
    }
    dsa_limits lim{};
    (void)dsa_get_limits(nullptr, &lim);
    DeviceBuffer<EndPlan> plan;
    DeviceBuffer<u64> wlen, rlen, gcount, woff, roff, goff;
    DeviceBuffer<Totals> tot;
    DeviceBuffer<uint8_t> tmp;
    DeviceBuffer<Seg> seg_win;
    DeviceBuffer<Seg64> seg_rem;
    DeviceBuffer<uint32_t> key, idx, skey, sidx;
    TASK_HIP(plan.reserve((size_t)E));
    for (auto* b : {&wlen, &rlen, &gcount, &woff, &roff, &goff}) TASK_HIP(b->reserve((size_t)E));
    TASK_HIP(tot.reserve(1));
    const Totals none{NONE, 0};
    TASK_HIP(hipMemcpyAsync(tot.p, &none, sizeof none, hipMemcpyHostToDevice, st));
    const ExonsView X = ex->view();
    // (1) plan
    hipLaunchKernelGGL(k_task_plan, dim3(grid_of(E)), dim3(BLOCK), 0, st, pairs, E, P, (const task_seq*)ref->seqs.p, X, lim.max_ref_len,
                       plan.p, wlen.p, rlen.p, tot.p);
    TASK_HIP(hipEventRecord(s->ev[2], st));
    // (2) count
    hipLaunchKernelGGL(k_task_regions<false>, dim3(grid_of(E * REGION_GROUP)), dim3(BLOCK), 0, st, (const EndPlan*)plan.p, E, X, pairs,
                       gcount.p, (const u64*)nullptr, (cand_region*)nullptr, (int64_t)0);
    TASK_HIP(hipEventRecord(s->ev[3], st));
    // (3) offsets and totals, in 64 bits
    struct Sum { DeviceBuffer<u64>*len, *off; } sums[3] = {{&wlen, &woff}, {&rlen, &roff}, {&gcount, &goff}};
    u64 last[3][2] = {};
    Totals got = none;
    for (int k = 0; k < 3; ++k) {
        TASK_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, sums[k].len->p, sums[k].off->p, (int)E, st); }));
        TASK_HIP(hipMemcpyAsync(&last[k][0], sums[k].off->p + (E - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        TASK_HIP(hipMemcpyAsync(&last[k][1], sums[k].len->p + (E - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    }
    TASK_HIP(hipMemcpyAsync(&got, tot.p, sizeof got, hipMemcpyDeviceToHost, st));
    TASK_HIP(hipEventRecord(s->ev[4], st));
    TASK_HIP(hipStreamSynchronize(st));
    TASK_HIP(hipGetLastError());
    if (got.long_window != NONE) return TASK_FAIL(DSA_E_LIMIT, "pair %u: reference window longer than %d", got.long_window, lim.max_ref_len);
    const u64 WB = last[0][0] + last[0][1], RB = last[1][0] + last[1][1], NR = last[2][0] + last[2][1];
    if (WB > (u64)INT32_MAX) return TASK_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 window bytes in one store (%llu)", WB);
    if (NR > (u64)INT32_MAX) return TASK_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 mate regions in one store (%llu)", NR);
    if (RB > (u64)E * (u64)INT32_MAX) return TASK_FAIL(DSA_E_DEVICE, "internal: %llu remainder bytes of %lld tasks", RB, (long long)n);
    s->windows.bytes_len = (int64_t)WB;
    s->tasks.rem_len = (int64_t)RB;
    s->n_regions = (int64_t)NR;
    TASK_HIP(s->windows.bytes.reserve((size_t)WB + SRC_PAD));
    TASK_HIP(s->tasks.rem.reserve((size_t)RB + SRC_PAD));
    TASK_HIP(s->regions.reserve((size_t)NR));
    TASK_HIP(hipMemsetAsync(s->windows.bytes.p + WB, 0, SRC_PAD, st));
    TASK_HIP(hipMemsetAsync(s->tasks.rem.p + RB, 0, SRC_PAD, st));
    // (4) emit
    hipLaunchKernelGGL(k_task_regions<true>, dim3(grid_of(E * REGION_GROUP)), dim3(BLOCK), 0, st, (const EndPlan*)plan.p, E, X, pairs,
                       (u64*)nullptr, (const u64*)goff.p, s->regions.p, (int64_t)NR);
    // (5) records, descriptors, gathers
    TASK_HIP(seg_win.reserve((size_t)E));
    TASK_HIP(seg_rem.reserve((size_t)E));
    for (auto* b : {&key, &idx, &skey, &sidx}) TASK_HIP(b->reserve((size_t)n));
    hipLaunchKernelGGL(k_task_records, dim3(grid_of(n)), dim3(BLOCK), 0, st, pairs, n, (const EndPlan*)plan.p, (const u64*)woff.p,
                       (const u64*)roff.p, (const u64*)goff.p, (const u64*)gcount.p, s->records.p, key.p, idx.p, seg_win.p, seg_rem.p);
    TASK_HIP(hipEventRecord(s->ev[5], st));
    hipLaunchKernelGGL((k_bat_gather<WINDOW_GROUP, true, Seg>), dim3(grid_of(E * WINDOW_GROUP)), dim3(BLOCK), 0, st, (const Seg*)seg_win.p, E,
                       (const uint8_t*)ref->bytes.p, ref->bytes_len, s->windows.bytes.p, (int64_t)WB);
    hipLaunchKernelGGL((k_bat_gather<REM_GROUP, true, Seg64>), dim3(grid_of(E * REM_GROUP)), dim3(BLOCK), 0, st, (const Seg64*)seg_rem.p, E,
                       (const uint8_t*)ref->bytes.p, ref->bytes_len, s->tasks.rem.p, (int64_t)RB);
    TASK_HIP(hipEventRecord(s->ev[6], st));
    // (6) the key order of the two stores
    TASK_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, (const uint32_t*)key.p, skey.p, (const uint32_t*)idx.p, sidx.p, (int)n, 0, 31, st);
    }));
    hipLaunchKernelGGL(k_task_stores, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const uint32_t*)skey.p, (const uint32_t*)sidx.p, n, (const task_record*)s->records.p,
                       (const EndPlan*)plan.p, s->windows.wkey.p, s->windows.wfus.p, s->tasks.tkey.p, s->tasks.task.p);
    TASK_HIP(hipEventRecord(s->ev[7], st));
    TASK_HIP(hipStreamSynchronize(st));
    TASK_HIP(hipGetLastError());
    task_timing& t = s->timing;
    t.upload_ms = hiphost::elapsed(s->ev[0], s->ev[1]);
    t.plan_ms = hiphost::elapsed(s->ev[1], s->ev[2]);
    t.count_ms = hiphost::elapsed(s->ev[2], s->ev[3]);
    t.scan_ms = hiphost::elapsed(s->ev[3], s->ev[4]);
    t.region_ms = hiphost::elapsed(s->ev[4], s->ev[5]);
    t.gather_ms = hiphost::elapsed(s->ev[5], s->ev[6]);
    t.sort_ms = hiphost::elapsed(s->ev[6], s->ev[7]);
    t.n_regions = (int64_t)NR;
    t.window_bytes = (int64_t)WB;
    t.rem_bytes = (int64_t)RB;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* task_last_error(void) { return g_task_err.c_str(); }

int task_reference_create(int device, const uint8_t* bytes, int64_t bytes_len, const task_seq* seqs, int64_t n_seqs, task_reference** out)
{
    if (!out) return TASK_FAIL(DSA_E_ARG, "task_reference_create: no output");
    *out = nullptr;
    if (const int rc = taskhost::check_reference(bytes, bytes_len, seqs, n_seqs, g_task_err)) return rc;
    if (hiphost::check_device(device, &g_task_err)) return DSA_E_DEVICE;
    TASK_HIP(hipSetDevice(device));
    task_reference* r = new task_reference();
    r->device = device;
    r->n_seqs = n_seqs;
    r->bytes_len = bytes_len;
    auto build = [&]() -> int {
        TASK_HIP(r->bytes.reserve((size_t)bytes_len + SRC_PAD));
        TASK_HIP(r->seqs.reserve((size_t)n_seqs));
        if (bytes_len) TASK_HIP(hipMemcpy(r->bytes.p, bytes, (size_t)bytes_len, hipMemcpyHostToDevice));
        TASK_HIP(hipMemset(r->bytes.p + bytes_len, 0, SRC_PAD));
        if (n_seqs) TASK_HIP(hipMemcpy(r->seqs.p, seqs, (size_t)n_seqs * sizeof(task_seq), hipMemcpyHostToDevice));
        TASK_HIP(hipDeviceSynchronize());
        return DSA_OK;
    };
    if (const int rc = build()) {
        delete r;
        return rc;
    }
    *out = r;
    return DSA_OK;
}

void task_reference_destroy(task_reference* r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

int task_exons_create(int device, const int32_t* chrom_ref, int32_t n_chroms, const task_transcript* transcripts, int32_t n_transcripts,
                      const task_exon* exons, int64_t n_exons, task_exons** out)
{
    if (!out) return TASK_FAIL(DSA_E_ARG, "task_exons_create: no output");
    *out = nullptr;
    taskhost::ExonIndex ix;
    if (const int rc = taskhost::build_exons(chrom_ref, n_chroms, transcripts, n_transcripts, exons, n_exons, ix, g_task_err)) return rc;
    if (hiphost::check_device(device, &g_task_err)) return DSA_E_DEVICE;
    TASK_HIP(hipSetDevice(device));
    task_exons* x = new task_exons();
    x->device = device;
    x->n_chroms = n_chroms;
    x->n_tx = n_transcripts;
    auto build = [&]() -> int {
        hipStream_t st = nullptr;
        if (const int rc = upload(x->tx, transcripts, (size_t)n_transcripts, st)) return rc;
        if (const int rc = upload(x->exons, exons, (size_t)n_exons, st)) return rc;
        if (const int rc = upload(x->chrom_ref, chrom_ref, (size_t)n_chroms, st)) return rc;
        struct Col { DeviceBuffer<int32_t>* dev; const std::vector<int32_t>* host; } cols[] = {
            {&x->tx_len, &ix.tx_len}, {&x->tx_reg, &ix.tx_reg}, {&x->chrom_bin_lo, &ix.chrom_bin_lo}, {&x->chrom_bins, &ix.chrom_bins},
            {&x->chrom_row, &ix.chrom_row}, {&x->row_first, &ix.row_first}, {&x->row_tx, &ix.row_tx}};
        for (const Col& c : cols)
            if (const int rc = upload(*c.dev, c.host->data(), c.host->size(), st)) return rc;
        TASK_HIP(hipStreamSynchronize(st));         // (the host columns are pageable: the copies are done, this is for the rule)
        return DSA_OK;
    };
    if (const int rc = build()) {
        (void)hipDeviceSynchronize();
        delete x;
        return rc;
    }
    *out = x;
    return DSA_OK;
}

void task_exons_destroy(task_exons* x)
{
    if (!x) return;
    (void)hipSetDevice(x->device);
    delete x;
}

int task_store_create(const task_reference* reference, const task_exons* exons, const task_params* params, const task_pair* pairs, int64_t n,
                      task_store** out)
{
    if (!out) return TASK_FAIL(DSA_E_ARG, "task_store_create: no output");
    *out = nullptr;
    if (const int rc = taskhost::check_params(params, g_task_err)) return rc;
    if (const int rc = taskhost::check_pairs(pairs, n, g_task_err)) return rc;
    if (!reference || !exons) return TASK_FAIL(DSA_E_ARG, "task_store_create: no %s", !reference ? "reference" : "exons");
    if (reference->device != exons->device)
        return TASK_FAIL(DSA_E_ARG, "task_store_create: the reference and the exons are on devices %d and %d", reference->device, exons->device);
    if (const int rc = taskhost::check_pair_indices(pairs, n, reference->n_seqs, exons->n_tx, exons->n_chroms, g_task_err)) return rc;
    TASK_HIP(hipSetDevice(reference->device));
    task_store* s = new task_store();
    s->device = reference->device;
    s->n = n;
    s->timing.n_tasks = n;
    DeviceBuffer<task_pair> dpairs;                 // (outlives the synchronise below)
    auto build = [&]() -> int {
        if (const int rc = open_store(s)) return rc;
        if (n) {
            TASK_HIP(hipEventRecord(s->ev[0], s->st));
            if (const int rc = upload(dpairs, pairs, (size_t)n, s->st)) return rc;
            TASK_HIP(hipEventRecord(s->ev[1], s->st));
        }
        return build_store(s, reference, exons, *params, dpairs.p, n);
    };
    if (const int rc = build()) {
        (void)hipStreamSynchronize(s->st);          // nothing of a refused call is in flight when it returns
        delete s;
        return rc;
    }
    *out = s;
    return DSA_OK;
}

void task_store_destroy(task_store* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    delete s;
}

const bat_windows* task_store_windows(const task_store* s) { return s ? &s->windows : nullptr; }

const pred_tasks* task_store_pred_tasks(const task_store* s) { return s ? &s->tasks : nullptr; }

int task_store_counts(const task_store* s, task_counts* out)
{
    if (!s || !out) return TASK_FAIL(DSA_E_ARG, "task_store_counts: no %s", !s ? "store" : "output");
    *out = task_counts{s->n, s->windows.bytes_len, s->tasks.rem_len, s->n_regions};
    return DSA_OK;
}

int task_store_fetch(task_store* s, task_record* records, int64_t records_cap, uint8_t* window_bytes, int64_t window_cap, uint8_t* rem_bytes,
                     int64_t rem_cap, cand_region* regions, int64_t regions_cap)
{
    if (!s) return TASK_FAIL(DSA_E_ARG, "task_store_fetch: no store");
    if (records_cap < 0 || window_cap < 0 || rem_cap < 0 || regions_cap < 0) return TASK_FAIL(DSA_E_ARG, "task_store_fetch: negative capacity");
    if ((records_cap && !records) || (window_cap && !window_bytes) || (rem_cap && !rem_bytes) || (regions_cap && !regions))
        return TASK_FAIL(DSA_E_ARG, "task_store_fetch: capacity without a buffer");
    // a part without a buffer is not wanted
    const int64_t need[4] = {records ? s->n : 0, window_bytes ? s->windows.bytes_len : 0, rem_bytes ? s->tasks.rem_len : 0, regions ? s->n_regions : 0};
    if (records_cap < need[0] || window_cap < need[1] || rem_cap < need[2] || regions_cap < need[3])
        return TASK_FAIL(DSA_E_CAPACITY, "the store has %lld tasks, %lld window bytes, %lld remainder bytes and %lld regions", (long long)s->n,
                         (long long)s->windows.bytes_len, (long long)s->tasks.rem_len, (long long)s->n_regions);
    TASK_HIP(hipSetDevice(s->device));
    hipStream_t st = s->st;
    TASK_HIP(hipEventRecord(s->ev[8], st));
    if (need[0]) TASK_HIP(hipMemcpyAsync(records, s->records.p, (size_t)need[0] * sizeof(task_record), hipMemcpyDeviceToHost, st));
    if (need[1]) TASK_HIP(hipMemcpyAsync(window_bytes, s->windows.bytes.p, (size_t)need[1], hipMemcpyDeviceToHost, st));
    if (need[2]) TASK_HIP(hipMemcpyAsync(rem_bytes, s->tasks.rem.p, (size_t)need[2], hipMemcpyDeviceToHost, st));
    if (need[3]) TASK_HIP(hipMemcpyAsync(regions, s->regions.p, (size_t)need[3] * sizeof(cand_region), hipMemcpyDeviceToHost, st));
    TASK_HIP(hipEventRecord(s->ev[9], st));
    TASK_HIP(hipStreamSynchronize(st));
    s->timing.download_ms = hiphost::elapsed(s->ev[8], s->ev[9]);
    return DSA_OK;
}

int task_store_get_timing(const task_store* s, task_timing* out)
{
    if (!s || !out) return TASK_FAIL(DSA_E_ARG, "task_store_get_timing: no %s", !s ? "store" : "output");
    *out = s->timing;
    return DSA_OK;
}

}  // extern "C"

// task_store_create for pairs that are in device memory already (taskt_api.hip): the argument checks that need no pairs, then
// the same build.  The pairs' own checks are the caller's; max_seq is the number of sequences their seq indices stay below.
__attribute__((visibility("hidden"))) int taskstore_create_device(int device, const task_reference* reference, const task_exons* exons, const task_params* params,
                                                                  const task_pair* pairs_device, int64_t n, int64_t max_seq, task_store** out)
{
    *out = nullptr;
    if (const int rc = taskhost::check_params(params, g_task_err)) return rc;
    if (!reference || !exons) return TASK_FAIL(DSA_E_ARG, "no %s", !reference ? "reference" : "exons");
    if (reference->device != device || exons->device != device)
        return TASK_FAIL(DSA_E_ARG, "the reference and the exons are on devices %d and %d, the pairs on %d", reference->device, exons->device, device);
    if (max_seq > reference->n_seqs)
        return TASK_FAIL(DSA_E_ARG, "the pairs' sequences are numbered below %lld, the reference has %lld", (long long)max_seq, (long long)reference->n_seqs);
    TASK_HIP(hipSetDevice(device));
    task_store* s = new task_store();
    s->device = device;
    s->n = n;
    s->timing.n_tasks = n;
    auto build = [&]() -> int {
        if (const int rc = open_store(s)) return rc;
        if (n) {
            TASK_HIP(hipEventRecord(s->ev[0], s->st));
            TASK_HIP(hipEventRecord(s->ev[1], s->st));
        }
        return build_store(s, reference, exons, *params, pairs_device, n);
    };
    if (const int rc = build()) {
        (void)hipStreamSynchronize(s->st);
        delete s;
        return rc;
    }
    *out = s;
    return DSA_OK;
}

// For conc_api.hip: where the sequences of a reference lie (device pointers, valid as long as it lives).
__attribute__((visibility("hidden"))) void task_reference_device(const task_reference* r, int* device, const uint8_t** bytes, int64_t* bytes_len,
                                                                 const task_seq** seqs, int64_t* n_seqs)
{
    *device = r->device;
    *bytes = r->bytes.p;
    *bytes_len = r->bytes_len;
    *seqs = r->seqs.p;
    *n_seqs = r->n_seqs;
}
