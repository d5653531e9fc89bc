// est_api.hip — EST islands of estislands on gfx950 (include/defuse_est.h): EstCatalog::SortAndMergeSegments
// (tools/EstCatalog.cpp:72-101) for all chromosomes at once, and the island lookup of FilterContainedInEstIslands (:103-173)
// for all breakpoint alignments at once.
//
// The sequential merge, on the segments of one chromosome sorted by start (cur = the first segment, then for every segment
// s, the first included: s.start > cur.end ? (emit cur, cur = s) : cur.end = max(cur.end, s.end); emit cur at the end).
//
// (1) Segments with end >= start only.  Claim: before segment i (i >= 1), cur.end = max(end_j, j < i).  For i = 1 it is
//     end_0 (segment 0 itself merges: start_0 <= end_0).  If start_i > cur.end a new island begins with end_i, and
//     end_i >= start_i > cur.end = max(end_j, j < i), so cur.end = max(end_j, j <= i); otherwise cur.end = max(cur.end, end_i)
//     is that maximum too.  So segment i begins an island iff i = 0 or start_i > the running max of the earlier ends of its
//     chromosome, and an island's end is the running max at its last segment.  Ties: in a group of equal starts every
//     segment but the first has start = s <= end of the first, so only the group's first can begin an island, and whether it
//     does depends only on the ends of earlier groups; an island ends before a group's first segment, i.e. after a whole
//     group, where the running max covers the same set of segments in any order.  So the islands do not depend on the order
//     of equal starts.
// (2) A degenerate segment d (end_d < start_d).  If start_d <= cur.end it changes nothing (max(cur.end, end_d) = cur.end).
//     If start_d > cur.end it is EFFECTIVE: it begins an island (start_d, end_d), and the next segment x, start_x >= start_d >
//     end_d, always begins another — a reset of the running max.  A degenerate first segment is effective against itself
//     (start_0 > end_0 = cur.end) and is emitted twice, as the reference's loop does.  Between resets (1) holds.  Whether
//     degenerate d_j is effective depends on the last effective d_i before it: cur.end = max(end_i, ends of the normal
//     segments between d_i and d_j), and end_i < start_i <= start_j, so d_j is effective iff start_j > max(P_{i+1}, ..., P_j)
//     with P_k = the max end of the normal segments between d_{k-1} and d_k.  The P_k are one segmented scan; the chain of
//     decisions is a short sequential loop per chromosome over the degenerate segments alone (k_est_chain).
//
// Device pipeline: 64-bit keys (chromosome << 32 | biased start), a stable radix sort of (key, end) — the canonical order
// (chromosome, start, input order) — then [degenerate segments only: P scan, compaction, k_est_chain], the segmented running
// max of end (heads: chromosome starts, effective degenerate segments and their successors), boundary marks, an exclusive sum
// for island slots, and one pass that writes island starts and ends.  Lookup: one thread per query, a binary search in its
// chromosome's island range, then the reference's forward walk.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_est.h"
#include "hip_host.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::grid_of;

thread_local std::string g_est_err;

#define EST_HIP(call) HIPHOST_TRY(g_est_err, call)

constexpr int BLOCK = 256;
constexpr long long NEG_INF = LLONG_MIN;

// an element of the segmented running max: a head starts a new segment
struct SegMax {
    long long v;
    int head;
    int pad_;
};
struct SegMaxOp {
    __host__ __device__ SegMax operator()(const SegMax& a, const SegMax& b) const
    {
        return SegMax{b.head ? b.v : (a.v > b.v ? a.v : b.v), a.head | b.head, 0};
    }
};

__device__ inline int key_chrom(unsigned long long k) { return (int)(k >> 32); }
__device__ inline int key_start(unsigned long long k) { return (int)((unsigned)k ^ 0x80000000u); }

__global__ void k_est_keys(const int32_t* __restrict__ chrom, const int32_t* __restrict__ start, unsigned long long* __restrict__ key, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    key[i] = ((unsigned long long)(unsigned)chrom[i] << 32) | (unsigned long long)((unsigned)start[i] ^ 0x80000000u);
}

// P scan input: heads at chromosome starts and after degenerate segments; normal segments contribute their end
__global__ void k_est_p_in(const unsigned long long* __restrict__ key, const int32_t* __restrict__ end, SegMax* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = key_start(key[i]), e = end[i];
    int head = i == 0;
    if (i > 0) head = key_chrom(key[i - 1]) != key_chrom(key[i]) || end[i - 1] < key_start(key[i - 1]);
    out[i] = SegMax{e >= s ? (long long)e : NEG_INF, head, 0};
}

// degenerate segments -> flags for their compaction
__global__ void k_est_deg_flag(const unsigned long long* __restrict__ key, const int32_t* __restrict__ end, uint32_t* __restrict__ flag, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && end[i] < key_start(key[i]) ? 1u : 0u;     // flag[n] = 0: the exclusive sum's last entry is the count
}

// the compact list of degenerate segments: sorted row index, chromosome, start and P (max end of the normal segments between
// the previous degenerate segment of the chromosome, or its first segment, and this one)
__global__ void k_est_deg_list(const unsigned long long* __restrict__ key, const SegMax* __restrict__ pin, const SegMax* __restrict__ pscan,
                               const uint32_t* __restrict__ flag,
                               const uint32_t* __restrict__ pos, int64_t n, uint32_t* __restrict__ d_row, int32_t* __restrict__ d_chrom,
                               int32_t* __restrict__ d_start, long long* __restrict__ d_p)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const uint32_t k = pos[i];
    const int c = key_chrom(key[i]);
    // pscan[i - 1] is the inclusive max up to i - 1; it belongs to this segment unless i is a head (of the scan's input)
    const bool head = pin[i].head != 0;
    d_row[k] = (uint32_t)i;
    d_chrom[k] = c;
    d_start[k] = key_start(key[i]);
    d_p[k] = head ? NEG_INF : pscan[i - 1].v;
}

// one thread per chromosome: the chain of effective degenerate segments (file comment, (2))
__global__ void k_est_chain(const uint32_t* __restrict__ d_row, const int32_t* __restrict__ d_chrom, const int32_t* __restrict__ d_start,
                            const long long* __restrict__ d_p, int64_t nd, int n_chrom, uint8_t* __restrict__ eff)
{
    const int c = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (c >= n_chrom) return;
    int64_t lo = 0, hi = nd;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (d_chrom[mid] < c) lo = mid + 1; else hi = mid;
    }
    long long run = NEG_INF;
    for (int64_t k = lo; k < nd && d_chrom[k] == c; ++k) {
        run = d_p[k] > run ? d_p[k] : run;
        if ((long long)d_start[k] > run) {
            eff[d_row[k]] = 1;
            run = NEG_INF;
        }
    }
}

// the running max of end: heads at chromosome starts, effective degenerate segments and the segment after one; normal and
// effective degenerate segments contribute their end, the others nothing
__global__ void k_est_m_in(const unsigned long long* __restrict__ key, const int32_t* __restrict__ end, const uint8_t* __restrict__ eff,
                           SegMax* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int s = key_start(key[i]), e = end[i];
    const bool ef = eff && eff[i];
    const bool head = i == 0 || key_chrom(key[i - 1]) != key_chrom(key[i]) || ef || (eff && eff[i - 1]);
    out[i] = SegMax{(e >= s || ef) ? (long long)e : NEG_INF, head ? 1 : 0, 0};
}

// island slots per segment: 1 where an island begins, 2 for a degenerate first segment of a chromosome, else 0
__global__ void k_est_mark(const unsigned long long* __restrict__ key, const int32_t* __restrict__ end, const uint8_t* __restrict__ eff,
                           const SegMax* __restrict__ m_in, const SegMax* __restrict__ m, uint32_t* __restrict__ cnt, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) { cnt[n] = 0; return; }
    const int s = key_start(key[i]);
    const bool first = i == 0 || key_chrom(key[i - 1]) != key_chrom(key[i]);
    uint32_t c;
    if (end[i] < s) c = (eff && eff[i]) ? (first ? 2u : 1u) : 0u;
    else c = (m_in[i].head || (long long)s > m[i - 1].v) ? 1u : 0u;      // a head covers i == 0
    cnt[i] = c;
}

// island k: start where it begins, end = the running max at its last segment
__global__ void k_est_emit(const unsigned long long* __restrict__ key, const int32_t* __restrict__ end, const SegMax* __restrict__ m,
                           const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off, int64_t n, int32_t* __restrict__ is,
                           int32_t* __restrict__ ie)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = off[i];
    const int s = key_start(key[i]);
    if (cnt[i]) is[o] = s;
    if (cnt[i] == 2) { is[o + 1] = s; ie[o] = end[i]; }
    const bool last = i + 1 == n || key_chrom(key[i + 1]) != key_chrom(key[i]) || cnt[i + 1] != 0;
    if (last) ie[off[i + 1] - 1] = (int32_t)m[i].v;
}

// chromosome c's islands begin at off[first segment of c] (off[n] = the count for chromosomes past the last segment)
__global__ void k_est_chrom_off(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ off, int64_t n, int n_chrom,
                                int64_t* __restrict__ chrom_off)
{
    const int c = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (c > n_chrom) return;
    const unsigned long long want = (unsigned long long)(unsigned)c << 32;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] < want) lo = mid + 1; else hi = mid;
    }
    chrom_off[c] = (int64_t)off[lo];
}

// the reference's lookup (tools/EstCatalog.cpp:141-167) for one query per thread
__global__ void k_est_lookup(const int32_t* __restrict__ is, const int32_t* __restrict__ ie, const int64_t* __restrict__ chrom_off, int n_chrom,
                             const int32_t* __restrict__ qc, const int32_t* __restrict__ qs, const int32_t* __restrict__ qe, int64_t n,
                             uint8_t* __restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const int c = qc[q];
    uint8_t res = 0;
    if (c >= 0 && c < n_chrom) {
        const int s = qs[q], e = qe[q];
        const int64_t first = chrom_off[c], last = chrom_off[c + 1];
        int64_t lo = first, hi = last;               // lower_bound: the first island with start >= s
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (is[mid] < s) lo = mid + 1; else hi = mid;
        }
        if (lo != first) --lo;
        for (int64_t k = lo; k < last && is[k] <= e; ++k) {
            if ((long long)is[k] - EST_ISLAND_PAD <= s && (long long)ie[k] + EST_ISLAND_PAD >= e) { res = 1; break; }    // the result is sticky
        }
    }
    out[q] = res;
}

}  // namespace

struct est_catalog {
    int device = -1;
    int n_chrom = 0;
    hiphost::Stream st;
    hiphost::Event ev[2];
    int64_t n_segments = 0, n_degenerate = 0, n_islands = 0;
    float build_ms = 0;
    DeviceBuffer<int32_t> is, ie;
    DeviceBuffer<int64_t> chrom_off;
    DeviceBuffer<int32_t> qc, qs, qe;
    DeviceBuffer<uint8_t> qout;
};

extern "C" {

const char* est_last_error(void) { return g_est_err.c_str(); }

static int est_build(est_catalog* cat, const int32_t* chrom, const int32_t* start, const int32_t* end, int64_t n)
{
    hipStream_t st = cat->st;
    const int n_chrom = cat->n_chrom;
    DeviceBuffer<int32_t> d_chrom, d_start, d_end, end_sorted;
    DeviceBuffer<unsigned long long> key, key_sorted;
    DeviceBuffer<SegMax> scan_in, scan_out;
    DeviceBuffer<uint32_t> cnt, off;
    DeviceBuffer<uint8_t> eff, tmp;
    EST_HIP(hipEventRecord(cat->ev[0], st));
    EST_HIP(cat->chrom_off.reserve((size_t)n_chrom + 1));
    if (n == 0) {
        EST_HIP(hipMemsetAsync(cat->chrom_off.p, 0, ((size_t)n_chrom + 1) * sizeof(int64_t), st));
        EST_HIP(hipEventRecord(cat->ev[1], st));
        EST_HIP(hipStreamSynchronize(st));
        cat->build_ms = hiphost::elapsed(cat->ev[0], cat->ev[1]);
        return DSA_OK;
    }
    EST_HIP(d_chrom.reserve((size_t)n));
    EST_HIP(d_start.reserve((size_t)n));
    EST_HIP(d_end.reserve((size_t)n));
    EST_HIP(end_sorted.reserve((size_t)n));
    EST_HIP(key.reserve((size_t)n));
    EST_HIP(key_sorted.reserve((size_t)n));
    EST_HIP(scan_in.reserve((size_t)n));
    EST_HIP(scan_out.reserve((size_t)n));
    EST_HIP(cnt.reserve((size_t)n + 1));
    EST_HIP(off.reserve((size_t)n + 1));
    EST_HIP(hipMemcpyAsync(d_chrom.p, chrom, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    EST_HIP(hipMemcpyAsync(d_start.p, start, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    EST_HIP(hipMemcpyAsync(d_end.p, end, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const unsigned g = grid_of(n), g1 = grid_of(n + 1);
    const int ni = (int)n;
    hipLaunchKernelGGL(k_est_keys, dim3(g), dim3(BLOCK), 0, st, d_chrom.p, d_start.p, key.p, n);
    int chrom_bits = 0;
    while (chrom_bits < 31 && ((int64_t)1 << chrom_bits) < n_chrom) ++chrom_bits;
    // stable: equal keys keep the input order, the canonical order of degenerate ties
    EST_HIP(hiphost::cub_run(tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceRadixSort::SortPairs(t, tb, key.p, key_sorted.p, d_end.p, end_sorted.p, ni, 0, 32 + chrom_bits, st);
    }));
    const unsigned long long* K = key_sorted.p;
    const int32_t* E = end_sorted.p;
    if (cat->n_degenerate) {
        EST_HIP(eff.reserve((size_t)n));
        EST_HIP(hipMemsetAsync(eff.p, 0, (size_t)n, st));
        hipLaunchKernelGGL(k_est_p_in, dim3(g), dim3(BLOCK), 0, st, K, E, scan_in.p, n);
        EST_HIP(hiphost::cub_run(tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceScan::InclusiveScan(t, tb, scan_in.p, scan_out.p, SegMaxOp(), ni, st);
        }));
        hipLaunchKernelGGL(k_est_deg_flag, dim3(g1), dim3(BLOCK), 0, st, K, E, cnt.p, n);
        EST_HIP(hiphost::cub_run(tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceScan::ExclusiveSum(t, tb, cnt.p, off.p, ni + 1, st);
        }));
        const int64_t nd = cat->n_degenerate;
        DeviceBuffer<uint32_t> d_row;
        DeviceBuffer<int32_t> dc, ds;
        DeviceBuffer<long long> dp;
        EST_HIP(d_row.reserve((size_t)nd));
        EST_HIP(dc.reserve((size_t)nd));
        EST_HIP(ds.reserve((size_t)nd));
        EST_HIP(dp.reserve((size_t)nd));
        uint32_t got = 0;
        EST_HIP(hipMemcpyAsync(&got, off.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        EST_HIP(hipStreamSynchronize(st));
        if ((int64_t)got != nd) { g_est_err = "internal: degenerate segment count differs from the host's"; return DSA_E_DEVICE; }
        hipLaunchKernelGGL(k_est_deg_list, dim3(g), dim3(BLOCK), 0, st, K, scan_in.p, scan_out.p, cnt.p, off.p, n, d_row.p, dc.p, ds.p, dp.p);
        hipLaunchKernelGGL(k_est_chain, dim3(grid_of(n_chrom)), dim3(BLOCK), 0, st, d_row.p, dc.p, ds.p, dp.p, nd, n_chrom, eff.p);
        EST_HIP(hipStreamSynchronize(st));           // (the compact list is freed on the way out of this block)
    }
    const uint8_t* EF = cat->n_degenerate ? eff.p : nullptr;
    hipLaunchKernelGGL(k_est_m_in, dim3(g), dim3(BLOCK), 0, st, K, E, EF, scan_in.p, n);
    EST_HIP(hiphost::cub_run(tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::InclusiveScan(t, tb, scan_in.p, scan_out.p, SegMaxOp(), ni, st);
    }));
    hipLaunchKernelGGL(k_est_mark, dim3(g1), dim3(BLOCK), 0, st, K, E, EF, scan_in.p, scan_out.p, cnt.p, n);
    EST_HIP(hiphost::cub_run(tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::ExclusiveSum(t, tb, cnt.p, off.p, ni + 1, st);
    }));
    uint32_t n_islands = 0;
    EST_HIP(hipMemcpyAsync(&n_islands, off.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    EST_HIP(hipStreamSynchronize(st));
    if (n_islands == 0 || (int64_t)n_islands > n + n_chrom) { g_est_err = "internal: island count out of range"; return DSA_E_DEVICE; }
    EST_HIP(cat->is.reserve(n_islands));
    EST_HIP(cat->ie.reserve(n_islands));
    hipLaunchKernelGGL(k_est_emit, dim3(g), dim3(BLOCK), 0, st, K, E, scan_out.p, cnt.p, off.p, n, cat->is.p, cat->ie.p);
    hipLaunchKernelGGL(k_est_chrom_off, dim3(grid_of((int64_t)n_chrom + 1)), dim3(BLOCK), 0, st, K, off.p, n, n_chrom, cat->chrom_off.p);
    EST_HIP(hipEventRecord(cat->ev[1], st));
    EST_HIP(hipStreamSynchronize(st));
    EST_HIP(hipGetLastError());
    cat->n_islands = n_islands;
    cat->build_ms = hiphost::elapsed(cat->ev[0], cat->ev[1]);
    return DSA_OK;
}

int est_catalog_create(int device, const int32_t* chrom, const int32_t* start, const int32_t* end, int64_t n, int32_t n_chrom,
                       est_catalog** out)
{
    if (!out) return DSA_E_ARG;
    *out = nullptr;
    if (n < 0 || n_chrom < 0 || (n && (!chrom || !start || !end))) return DSA_E_ARG;
    // 32-bit scans and slots (n + n_chrom islands at most: a degenerate first segment counts twice)
    if (n >= INT32_MAX - 1 || n + (int64_t)n_chrom >= (int64_t)UINT32_MAX) { g_est_err = "more than 2^31 - 2 EST segments in one catalogue"; return DSA_E_LIMIT; }
    int64_t n_deg = 0;
    for (int64_t k = 0; k < n; ++k) {
        if (chrom[k] < 0 || chrom[k] >= n_chrom) { g_est_err = "chromosome id out of range at segment " + std::to_string(k); return DSA_E_ARG; }
        n_deg += end[k] < start[k];
    }
    if (hiphost::check_device(device, &g_est_err)) return DSA_E_DEVICE;
    EST_HIP(hipSetDevice(device));
    est_catalog* cat = new est_catalog();
    cat->device = device;
    cat->n_chrom = n_chrom;
    cat->n_segments = n;
    cat->n_degenerate = n_deg;
    if (cat->st.create(hipStreamNonBlocking) != hipSuccess || cat->ev[0].create() != hipSuccess || cat->ev[1].create() != hipSuccess) {
        delete cat;
        g_est_err = "cannot create a stream";
        return DSA_E_DEVICE;
    }
    const int rc = est_build(cat, chrom, start, end, n);
    if (rc != DSA_OK) {
        delete cat;
        return rc;
    }
    *out = cat;
    return DSA_OK;
}

int est_catalog_islands(est_catalog* cat, int32_t* start, int32_t* end, int64_t cap, int64_t* n_islands, int64_t* chrom_off)
{
    if (!cat || !n_islands) return DSA_E_ARG;
    *n_islands = cat->n_islands;
    if (cat->n_islands > cap) return DSA_E_CAPACITY;
    if ((cat->n_islands && (!start || !end)) || !chrom_off) return DSA_E_ARG;
    EST_HIP(hipSetDevice(cat->device));
    if (cat->n_islands) {
        EST_HIP(hipMemcpy(start, cat->is.p, (size_t)cat->n_islands * sizeof(int32_t), hipMemcpyDeviceToHost));
        EST_HIP(hipMemcpy(end, cat->ie.p, (size_t)cat->n_islands * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    EST_HIP(hipMemcpy(chrom_off, cat->chrom_off.p, ((size_t)cat->n_chrom + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return DSA_OK;
}

int est_catalog_contained(est_catalog* cat, const int32_t* chrom, const int32_t* start, const int32_t* end, int64_t n,
                          uint8_t* contained, est_timing* timing)
{
    if (!cat || n < 0 || (n && (!chrom || !start || !end || !contained))) return DSA_E_ARG;
    EST_HIP(hipSetDevice(cat->device));
    hipStream_t st = cat->st;
    float ms = 0;
    if (n) {
        EST_HIP(cat->qc.reserve((size_t)n));
        EST_HIP(cat->qs.reserve((size_t)n));
        EST_HIP(cat->qe.reserve((size_t)n));
        EST_HIP(cat->qout.reserve((size_t)n));
        EST_HIP(hipEventRecord(cat->ev[0], st));
        EST_HIP(hipMemcpyAsync(cat->qc.p, chrom, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        EST_HIP(hipMemcpyAsync(cat->qs.p, start, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        EST_HIP(hipMemcpyAsync(cat->qe.p, end, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_est_lookup, dim3(grid_of(n)), dim3(BLOCK), 0, st, cat->is.p, cat->ie.p, cat->chrom_off.p, cat->n_chrom,
                           cat->qc.p, cat->qs.p, cat->qe.p, n, cat->qout.p);
        EST_HIP(hipMemcpyAsync(contained, cat->qout.p, (size_t)n, hipMemcpyDeviceToHost, st));
        EST_HIP(hipEventRecord(cat->ev[1], st));
        EST_HIP(hipStreamSynchronize(st));
        EST_HIP(hipGetLastError());
        ms = hiphost::elapsed(cat->ev[0], cat->ev[1]);
    }
    if (timing) {
        int64_t hit = 0;
        for (int64_t k = 0; k < n; ++k) hit += contained[k] != 0;
        *timing = est_timing{cat->build_ms, ms, cat->n_segments, cat->n_degenerate, cat->n_islands, n, hit};
    }
    return DSA_OK;
}

void est_catalog_destroy(est_catalog* cat)
{
    if (!cat) return;
    (void)hipSetDevice(cat->device);
    (void)hipStreamSynchronize(cat->st);
    delete cat;
}

}  // extern "C"
