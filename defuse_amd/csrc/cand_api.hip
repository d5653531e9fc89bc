// cand_api.hip — the candidate loop of SplitReadRealigner::DoAlignment on gfx950 (include/defuse_cand.h):
// BinnedLocations::Add / Overlapping (tools/SplitAlignment.cpp:177-229) for all mate regions and all improper mate
// alignments of a call at once, and candidateUnique (:268, :292) as a sorted array of 64-bit keys per session.
//
// Table (cand_table_create).  Every (region, bin) entry gets the key (strand << 63 | ref << 32 | biased bin) and the region
// index as payload; one stable radix sort groups the entries of a bin, and the distinct keys with the offsets of their runs
// are the lookup table.  The entries of a (strand, ref) are contiguous and ascending in bin, so the bins bin0..bin1 of an
// alignment are ONE range of entries between two binary searches — a range of bins the table does not have costs nothing.
//
// Enumeration (cand_enumerate), all on the session's stream, nothing ordered by an atomic:
//   (1) one thread per alignment counts the entries of its range that pass the overlap test, a 64-bit exclusive sum gives
//       each alignment its slot, and the same walk writes (alignment << 32 | biased id) keys there;
//   (2) a radix sort and a head-flag compaction leave the distinct (alignment, id) in ascending order: the visiting order;
//   (3) each visited hit becomes the 64-bit candidate key fusion << 33 | fragment << 2 | read_end << 1 | revcomp
//       (31 + 31 + 1 + 1 bits).  A STABLE sort of (key, visiting rank) puts the first-visited of equal keys at the head of
//       its run; that one is kept unless a binary search finds the key in the session's sorted seen keys;
//   (4) the keep flags go back to visiting rank, an exclusive sum compacts the kept candidates into records; a stable sort
//       by fusion id reorders them for CAND_ORDER_FUSION;
//   (5) only when the records fit the caller's buffer are the new keys (already sorted, distinct, disjoint from the seen
//       ones) merged into the seen array, each element placed by its rank in the other array.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <string>

#include "../../include/defuse_bat.h"      // cand_enumerate_device, cand_records_device
#include "../../include/defuse_cand.h"
#include "../../include/defuse_dsa.h"
#include "../../include/defuse_text.h"     // cand_enumerate_resident
#include "hip_host.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using u64 = unsigned long long;

thread_local std::string g_cand_err;

#define CAND_HIP(call) HIPHOST_TRY(g_cand_err, call)
#define CAND_FAIL(code, ...) hiphost::fail(g_cand_err, code, __VA_ARGS__)

constexpr int BLOCK = 256;

// C++ int division truncates toward zero; spacing > 0, so no quotient overflows
__host__ __device__ inline int bin_of(int x, int spacing) { return x / spacing; }
__host__ __device__ inline u64 bin_key(int strand, int ref, int bin)
{
    return ((u64)(unsigned)strand << 63) | ((u64)(unsigned)ref << 32) | (u64)((unsigned)bin ^ 0x80000000u);
}

// the first index in [0, n) with a[index] >= x (UPPER: > x)
template <bool UPPER, typename T>
__device__ inline int64_t bound(const T* __restrict__ a, int64_t n, T x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (UPPER ? a[mid] <= x : a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- table ------------------------------------------------------------------------------------------------------------

// bins per region (the host has checked that their sum, and so each of them, is below 2^31)
__global__ void k_tab_count(const cand_region* __restrict__ reg, int64_t n, int spacing, uint32_t* __restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int b0 = bin_of(reg[i].start, spacing), b1 = bin_of(reg[i].end, spacing);
    cnt[i] = b0 <= b1 ? (uint32_t)((int64_t)b1 - b0 + 1) : 0u;
}

// one thread per entry: its region is the last one whose offset is <= e (regions without bins share the next one's offset)
__global__ void k_tab_emit(const cand_region* __restrict__ reg, const uint32_t* __restrict__ off, int64_t n, int spacing, int64_t n_entries,
                           u64* __restrict__ key, uint32_t* __restrict__ region)
{
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= n_entries) return;
    const int64_t r = bound<true>(off, n, (uint32_t)e) - 1;
    const cand_region g = reg[r];
    const int bin = (int)((int64_t)bin_of(g.start, spacing) + (e - (int64_t)off[r]));
    key[e] = bin_key(g.strand, g.ref, bin);
    region[e] = (uint32_t)r;
}

__global__ void k_heads(const u64* __restrict__ key, int64_t n, uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// distinct keys and where their runs begin; uoff[n_unique] = the number of entries
__global__ void k_tab_unique(const u64* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, int64_t n_entries,
                             int64_t n_unique, u64* __restrict__ ukey, uint32_t* __restrict__ uoff)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) uoff[n_unique] = (uint32_t)n_entries;
    if (i >= n_entries || !flag[i] || (int64_t)pos[i] >= n_unique) return;
    ukey[pos[i]] = key[i];
    uoff[pos[i]] = (uint32_t)i;
}

struct TabView {
    const cand_region* reg;
    const u64* ukey;            // n_unique distinct (strand, ref, bin), ascending
    const uint32_t* uoff;       // n_unique + 1 run offsets into ereg
    const uint32_t* ereg;       // region index of every entry
    int64_t n_unique;
    int spacing;
};

// ---- enumeration ------------------------------------------------------------------------------------------------------

// BinnedLocations::Overlapping without the set: WRITE = false counts alignment k's raw hits, WRITE = true writes their keys
// into its slot (the same walk, so the same number)
template <bool WRITE>
__global__ void k_cand_hits(TabView t, const cand_alignment* __restrict__ al, int64_t n, u64* __restrict__ cnt, const u64* __restrict__ off,
                            u64* __restrict__ key, int64_t n_hits)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const cand_alignment a = al[k];
    u64 c = 0;
    const int b0 = bin_of(a.start, t.spacing), b1 = bin_of(a.end, t.spacing);
    if (a.ref >= 0 && b0 <= b1 && t.n_unique > 0) {
        const int64_t lo = bound<false>(t.ukey, t.n_unique, bin_key(a.strand, a.ref, b0));
        const int64_t hi = bound<true>(t.ukey, t.n_unique, bin_key(a.strand, a.ref, b1));
        if (lo < hi) {
            const u64 base = WRITE ? off[k] : 0;
            const uint32_t e1 = t.uoff[hi];
            for (uint32_t e = t.uoff[lo]; e < e1; ++e) {
                const cand_region g = t.reg[t.ereg[e]];
                if (g.start <= a.end && g.end >= a.start) {
                    if (WRITE && base + c < (u64)n_hits) key[base + c] = ((u64)k << 32) | (u64)((unsigned)g.id ^ 0x80000000u);
                    ++c;
                }
            }
        }
    }
    if (!WRITE) cnt[k] = c;
}

// check_alignments for alignments that are on the device.  bad[0]: the lowest index with a strand or read end outside 0 / 1;
// bad[1]: the lowest with fragment < 0 that overlaps something (cnt from k_cand_hits<false>) - one that overlaps nothing
// is never cast by the reference either (tools/SplitAlignment.cpp:281 is inside the loop over the overlapping ids).
__global__ void k_cand_check(const cand_alignment* __restrict__ al, const u64* __restrict__ cnt, int64_t n, uint32_t* __restrict__ bad)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const cand_alignment a = al[k];
    if ((a.strand != 0 && a.strand != 1) || (a.read_end != 0 && a.read_end != 1)) atomicMin(&bad[0], (uint32_t)k);
    if (a.fragment < 0 && cnt[k] != 0) atomicMin(&bad[1], (uint32_t)k);
}

__device__ inline int hit_id(u64 key) { return (int)((unsigned)key ^ 0x80000000u); }

// the distinct hits in visiting order, and the candidate key of each (tools/SplitAlignment.cpp:281-284)
__global__ void k_cand_visit(const u64* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, int64_t n_hits,
                             int64_t n_visited, const cand_alignment* __restrict__ al, u64* __restrict__ vkey, u64* __restrict__ ckey,
                             uint32_t* __restrict__ rank)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_hits || !flag[i] || (int64_t)pos[i] >= n_visited) return;
    const uint32_t v = pos[i];
    const u64 h = key[i];
    const cand_alignment a = al[h >> 32];
    const int id = hit_id(h);
    const u64 fusion = (u64)((unsigned)id & 0x7FFFFFFFu);
    const u64 read_end = a.read_end == 0 ? 1 : 0;
    const u64 revcomp = id < 0 ? 0 : 1;
    vkey[v] = h;
    ckey[v] = (fusion << 33) | ((u64)(unsigned)a.fragment << 2) | (read_end << 1) | revcomp;
    rank[v] = v;
}

// in the order of the stable sort by candidate key: kept = head of its run and not seen before.  keep_v is indexed by
// visiting rank, keep_s by sorted position (for the new seen keys).
__global__ void k_cand_keep(const u64* __restrict__ cs, const uint32_t* __restrict__ rs, int64_t n_visited, const u64* __restrict__ seen,
                            int64_t n_seen, uint32_t* __restrict__ keep_v, uint32_t* __restrict__ keep_s)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_visited) return;
    const u64 c = cs[i];
    uint32_t keep = (i == 0 || cs[i - 1] != c) ? 1u : 0u;
    if (keep && n_seen) {
        const int64_t p = bound<false>(seen, n_seen, c);
        if (p < n_seen && seen[p] == c) keep = 0;
    }
    keep_s[i] = keep;
    if ((int64_t)rs[i] < n_visited) keep_v[rs[i]] = keep;
}

__global__ void k_cand_emit(const u64* __restrict__ vkey, const u64* __restrict__ ckey, const uint32_t* __restrict__ keep_v,
                            const uint32_t* __restrict__ kpos, int64_t n_visited, int64_t n_kept, int64_t given, cand_record* __restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_visited || !keep_v[i] || (int64_t)kpos[i] >= n_kept) return;
    const u64 h = vkey[i], c = ckey[i];
    cand_record r;
    r.alignment = given + (int64_t)(h >> 32);
    r.fusion_id = (int32_t)(c >> 33);
    r.fragment = (int32_t)((c >> 2) & 0x7FFFFFFFu);
    r.cluster_end = hit_id(h) < 0 ? 1 : 0;
    r.read_end = (uint8_t)((c >> 1) & 1);
    r.revcomp = (uint8_t)(c & 1);
    r.first = 0;
    r.pad_[0] = r.pad_[1] = r.pad_[2] = r.pad_[3] = 0;
    rec[kpos[i]] = r;
}

// records are in visiting order here: the first of an alignment follows a record of another one (only `first` is written,
// only `alignment` is read from the neighbour).  Also the sort input of CAND_ORDER_FUSION.
__global__ void k_cand_first(cand_record* rec, int64_t n_kept, uint32_t* __restrict__ fkey, uint32_t* __restrict__ idx)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_kept) return;
    rec[p].first = (p == 0 || rec[p - 1].alignment != rec[p].alignment) ? 1 : 0;
    fkey[p] = (uint32_t)rec[p].fusion_id;
    idx[p] = (uint32_t)p;
}

__global__ void k_cand_gather(const cand_record* __restrict__ rec, const uint32_t* __restrict__ idx, int64_t n_kept, cand_record* __restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n_kept || (int64_t)idx[p] >= n_kept) return;
    out[p] = rec[idx[p]];
}

__global__ void k_cand_newkeys(const u64* __restrict__ cs, const uint32_t* __restrict__ keep_s, const uint32_t* __restrict__ spos,
                               int64_t n_visited, int64_t n_kept, u64* __restrict__ nk)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_visited || !keep_s[i] || (int64_t)spos[i] >= n_kept) return;
    nk[spos[i]] = cs[i];
}

// two sorted arrays without a common element: each element goes to its own index plus its rank in the other array
__global__ void k_cand_merge(const u64* __restrict__ a, int64_t na, const u64* __restrict__ b, int64_t nb, u64* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= na + nb) return;
    if (t < na) out[t + bound<false>(b, nb, a[t])] = a[t];
    else out[(t - na) + bound<false>(a, na, b[t - na])] = b[t - na];
}

int bits_for(int64_t n)      // bits that hold 0 .. n - 1
{
    int b = 0;
    while (b < 63 && ((int64_t)1 << b) < n) ++b;
    return b;
}

}  // namespace

struct cand_table {
    int device = -1;
    int spacing = 0;
    int64_t n_regions = 0, n_entries = 0, n_unique = 0;
    hiphost::Stream st;
    DeviceBuffer<cand_region> reg;
    DeviceBuffer<u64> ukey;
    DeviceBuffer<uint32_t> uoff, ereg;
    TabView view() const { return TabView{reg.p, ukey.p, uoff.p, ereg.p, n_unique, spacing}; }
};

struct cand_session {
    cand_table* table = nullptr;
    int64_t given = 0;           // alignments of the calls that succeeded
    int64_t n_seen = 0;          // keys in `seen`, ascending
    hiphost::Stream st;
    hiphost::Event ev[4];
    DeviceBuffer<u64, GrowSize> seen, seen_next;
    // per call
    DeviceBuffer<cand_alignment, GrowSize> al;
    DeviceBuffer<u64, GrowSize> cnt, off, key, key_sorted, vkey, ckey, ckey_sorted, new_keys;
    DeviceBuffer<uint32_t, GrowSize> flag, pos, rank, rank_sorted, keep_v, keep_s, kpos, fkey, fkey_sorted, idx, idx_sorted;
    DeviceBuffer<cand_record, GrowSize> rec, rec_sorted;
    DeviceBuffer<uint8_t, GrowSize> tmp;
    DeviceBuffer<uint32_t> bad;                  // cand_enumerate_resident: k_cand_check's two indices
    // the records of the latest cand_enumerate_device (in rec or rec_sorted), until the next call on the session
    const cand_record* resident = nullptr;
    int64_t n_resident = 0;
};

namespace {

// the sum of flag[0..n) after its exclusive sum went to pos: pos[n - 1] + flag[n - 1]
int flag_total(hipStream_t st, const uint32_t* flag, const uint32_t* pos, int64_t n, int64_t* total)
{
    uint32_t last[2] = {0, 0};
    CAND_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CAND_HIP(hipMemcpyAsync(&last[1], flag + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CAND_HIP(hipStreamSynchronize(st));
    *total = (int64_t)last[0] + (int64_t)last[1];
    return DSA_OK;
}

int table_build(cand_table* t, const cand_region* regions)
{
    hipStream_t st = t->st;
    const int64_t n = t->n_regions, E = t->n_entries;
    CAND_HIP(t->reg.reserve((size_t)n));
    CAND_HIP(t->ukey.reserve(1));
    CAND_HIP(t->uoff.reserve(1));
    CAND_HIP(t->ereg.reserve((size_t)E));
    if (n) CAND_HIP(hipMemcpyAsync(t->reg.p, regions, (size_t)n * sizeof(cand_region), hipMemcpyHostToDevice, st));
    if (E == 0) {
        CAND_HIP(hipMemsetAsync(t->uoff.p, 0, sizeof(uint32_t), st));
        CAND_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    }
    DeviceBuffer<uint32_t> cnt, off, ereg_in, flag, pos;
    DeviceBuffer<u64> key, key_sorted;
    DeviceBuffer<uint8_t> tmp;
    CAND_HIP(cnt.reserve((size_t)n));
    CAND_HIP(off.reserve((size_t)n));
    CAND_HIP(ereg_in.reserve((size_t)E));
    CAND_HIP(flag.reserve((size_t)E));
    CAND_HIP(pos.reserve((size_t)E));
    CAND_HIP(key.reserve((size_t)E));
    CAND_HIP(key_sorted.reserve((size_t)E));
    hipLaunchKernelGGL(k_tab_count, dim3(grid_of(n)), dim3(BLOCK), 0, st, t->reg.p, n, t->spacing, cnt.p);
    CAND_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, cnt.p, off.p, (int)n, st); }));
    hipLaunchKernelGGL(k_tab_emit, dim3(grid_of(E)), dim3(BLOCK), 0, st, t->reg.p, off.p, n, t->spacing, E, key.p, ereg_in.p);
    // stable: the entries of a bin keep the order of the regions, as the reference's vectors do
    CAND_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, key.p, key_sorted.p, ereg_in.p, t->ereg.p, (int)E, 0, 64, st);
    }));
    hipLaunchKernelGGL(k_heads, dim3(grid_of(E)), dim3(BLOCK), 0, st, key_sorted.p, E, flag.p);
    CAND_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, flag.p, pos.p, (int)E, st); }));
    int64_t U = 0;
    if (const int rc = flag_total(st, flag.p, pos.p, E, &U)) return rc;
    if (U < 1 || U > E) return CAND_FAIL(DSA_E_DEVICE, "internal: %lld distinct bins of %lld entries", (long long)U, (long long)E);
    CAND_HIP(t->ukey.reserve((size_t)U));
    CAND_HIP(t->uoff.reserve((size_t)U + 1));
    hipLaunchKernelGGL(k_tab_unique, dim3(grid_of(E)), dim3(BLOCK), 0, st, key_sorted.p, flag.p, pos.p, E, U, t->ukey.p, t->uoff.p);
    CAND_HIP(hipStreamSynchronize(st));
    CAND_HIP(hipGetLastError());
    t->n_unique = U;
    return DSA_OK;
}

int check_alignments(const cand_alignment* al, int64_t n)
{
    for (int64_t k = 0; k < n; ++k) {
        if (al[k].strand != 0 && al[k].strand != 1) return CAND_FAIL(DSA_E_ARG, "alignment %lld: strand %d is not 0 or 1", (long long)k, al[k].strand);
        if (al[k].read_end != 0 && al[k].read_end != 1) return CAND_FAIL(DSA_E_ARG, "alignment %lld: read_end %d is not 0 or 1", (long long)k, al[k].read_end);
        if (al[k].fragment < 0) return CAND_FAIL(DSA_E_ARG, "alignment %lld: fragment %d is outside [0, 2^31)", (long long)k, al[k].fragment);
    }
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* cand_last_error(void) { return g_cand_err.c_str(); }

int cand_cluster_id(int64_t fusion_id, int32_t cluster_end, int32_t* id)
{
    if (!id) return CAND_FAIL(DSA_E_ARG, "cand_cluster_id: no output");
    if (fusion_id < 0 || fusion_id > (int64_t)INT32_MAX) return CAND_FAIL(DSA_E_ARG, "fusion id %lld is outside [0, 2^31)", (long long)fusion_id);
    if (cluster_end != 0 && cluster_end != 1) return CAND_FAIL(DSA_E_ARG, "cluster end %d is not 0 or 1", cluster_end);
    *id = (int32_t)((uint32_t)fusion_id | ((uint32_t)cluster_end << 31));
    return DSA_OK;
}

int cand_table_create(int device, const cand_region* regions, int64_t n, int32_t bin_spacing, cand_table** out)
{
    if (!out) return CAND_FAIL(DSA_E_ARG, "cand_table_create: no output");
    *out = nullptr;
    if (bin_spacing <= 0) return CAND_FAIL(DSA_E_ARG, "bin_spacing %d is not positive", bin_spacing);
    if (n < 0) return CAND_FAIL(DSA_E_ARG, "negative number of regions (%lld)", (long long)n);
    if (n > (int64_t)INT32_MAX) return CAND_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 mate regions in one table");
    if (n && !regions) return CAND_FAIL(DSA_E_ARG, "cand_table_create: no regions");
    int64_t entries = 0;     // 64 bits: one region can span 2^32 bins
    for (int64_t k = 0; k < n; ++k) {
        const cand_region& g = regions[k];
        if (g.ref < 0) return CAND_FAIL(DSA_E_ARG, "region %lld: reference index %d is negative", (long long)k, g.ref);
        if (g.strand != 0 && g.strand != 1) return CAND_FAIL(DSA_E_ARG, "region %lld: strand %d is not 0 or 1", (long long)k, g.strand);
        const int b0 = bin_of(g.start, bin_spacing), b1 = bin_of(g.end, bin_spacing);
        if (b0 <= b1) entries += (int64_t)b1 - b0 + 1;       // n < 2^31 regions of at most 2^32 bins: no overflow
    }
    if (entries > (int64_t)INT32_MAX)
        return CAND_FAIL(DSA_E_LIMIT, "%lld (region, bin) entries at bin spacing %d: more than 2^31 - 1", (long long)entries, bin_spacing);
    if (hiphost::check_device(device, &g_cand_err)) return DSA_E_DEVICE;
    CAND_HIP(hipSetDevice(device));
    cand_table* t = new cand_table();
    t->device = device;
    t->spacing = bin_spacing;
    t->n_regions = n;
    t->n_entries = entries;
    int rc = DSA_OK;
    if (t->st.create(hipStreamNonBlocking) != hipSuccess) rc = CAND_FAIL(DSA_E_DEVICE, "cannot create a stream");
    if (rc == DSA_OK) rc = table_build(t, regions);
    if (rc != DSA_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return DSA_OK;
}

void cand_table_destroy(cand_table* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->st);
    delete t;
}

int cand_session_create(cand_table* table, cand_session** out)
{
    if (!out) return CAND_FAIL(DSA_E_ARG, "cand_session_create: no output");
    *out = nullptr;
    if (!table) return CAND_FAIL(DSA_E_ARG, "cand_session_create: no table");
    CAND_HIP(hipSetDevice(table->device));
    cand_session* s = new cand_session();
    s->table = table;
    bool ok = s->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : s->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete s;
        return CAND_FAIL(DSA_E_DEVICE, "cannot create a stream");
    }
    *out = s;
    return DSA_OK;
}

int cand_session_reset(cand_session* s)
{
    if (!s) return CAND_FAIL(DSA_E_ARG, "cand_session_reset: no session");
    s->given = 0;
    s->n_seen = 0;
    return DSA_OK;
}

void cand_session_destroy(cand_session* s)
{
    if (!s) return;
    (void)hipSetDevice(s->table->device);
    (void)hipStreamSynchronize(s->st);
    delete s;
}

}  // extern "C"

namespace {

// cand_enumerate (RESIDENT = false: the records go to `out` if they fit cap) and cand_enumerate_device (true: they stay in
// the session's buffer, nothing is downloaded and no capacity is asked for).  DEVICE_SRC (cand_enumerate_resident): the
// alignments are in device memory of the session's GPU, a kernel checks them and *first_bad receives what it found.
template <bool RESIDENT, bool DEVICE_SRC = false>
int enumerate(cand_session* s, const cand_alignment* alignments, int64_t n, int32_t order, cand_record* out, int64_t cap, int64_t* n_out,
              cand_timing* timing, int64_t* first_bad = nullptr)
{
    if (!n_out) return CAND_FAIL(DSA_E_ARG, "cand_enumerate: no n_out");
    *n_out = 0;
    if (first_bad) *first_bad = -1;
    if (s) {
        s->resident = nullptr;
        s->n_resident = 0;
    }
    if (n < 0) return CAND_FAIL(DSA_E_ARG, "negative number of alignments (%lld)", (long long)n);
    if (n > (int64_t)INT32_MAX) return CAND_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 alignments in one call");
    if (n && !alignments) return CAND_FAIL(DSA_E_ARG, "cand_enumerate: no alignments");
    if (order != CAND_ORDER_VISIT && order != CAND_ORDER_FUSION) return CAND_FAIL(DSA_E_ARG, "order %d is neither CAND_ORDER_VISIT nor CAND_ORDER_FUSION", order);
    if (cap < 0 || (cap && !out)) return CAND_FAIL(DSA_E_ARG, "cand_enumerate: capacity %lld without a buffer", (long long)cap);
    if (!DEVICE_SRC)
        if (const int rc = check_alignments(alignments, n)) return rc;
    if (!s) return CAND_FAIL(DSA_E_ARG, "cand_enumerate: no session");

    if (timing) *timing = cand_timing{0, 0, 0, 0, n, 0, 0, 0};
    if (n == 0) return DSA_OK;
    const cand_table* t = s->table;
    CAND_HIP(hipSetDevice(t->device));
    hipStream_t st = s->st;
    const unsigned gn = grid_of(n);
    int64_t H = 0, V = 0, K = 0;

    CAND_HIP(s->al.reserve((size_t)n));
    CAND_HIP(s->cnt.reserve((size_t)n));
    CAND_HIP(s->off.reserve((size_t)n));
    CAND_HIP(s->key.reserve(1));
    CAND_HIP(hipEventRecord(s->ev[0], st));
    CAND_HIP(hipMemcpyAsync(s->al.p, alignments, (size_t)n * sizeof(cand_alignment), DEVICE_SRC ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    CAND_HIP(hipEventRecord(s->ev[1], st));

    // (1) raw hits
    hipLaunchKernelGGL(k_cand_hits<false>, dim3(gn), dim3(BLOCK), 0, st, t->view(), s->al.p, n, s->cnt.p, (const u64*)s->off.p, s->key.p, (int64_t)0);
    CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, s->cnt.p, s->off.p, (int)n, st); }));
    uint32_t bad[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    if (DEVICE_SRC) {
        CAND_HIP(s->bad.reserve(2));
        CAND_HIP(hipMemcpyAsync(s->bad.p, bad, sizeof bad, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_cand_check, dim3(gn), dim3(BLOCK), 0, st, (const cand_alignment*)s->al.p, (const u64*)s->cnt.p, n, s->bad.p);
        CAND_HIP(hipMemcpyAsync(bad, s->bad.p, sizeof bad, hipMemcpyDeviceToHost, st));
    }
    {
        u64 last[2] = {0, 0};
        CAND_HIP(hipMemcpyAsync(&last[0], s->off.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        CAND_HIP(hipMemcpyAsync(&last[1], s->cnt.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
        CAND_HIP(hipStreamSynchronize(st));
        CAND_HIP(hipGetLastError());
        if (DEVICE_SRC && (int64_t)bad[0] < n) return CAND_FAIL(DSA_E_ARG, "alignment %u: strand or read_end is not 0 or 1", bad[0]);
        if (DEVICE_SRC && (int64_t)bad[1] < n) {
            if (first_bad) *first_bad = (int64_t)bad[1];
            return CAND_FAIL(DSA_E_ARG, "alignment %u: its fragment is outside [0, 2^31) and it overlaps a mate region", bad[1]);
        }
        if (last[0] + last[1] > (u64)INT32_MAX)
            return CAND_FAIL(DSA_E_LIMIT, "%llu overlaps in one call: more than 2^31 - 1, give fewer alignments per call", last[0] + last[1]);
        H = (int64_t)(last[0] + last[1]);
    }
    if (H) {
        const unsigned gh = grid_of(H);
        CAND_HIP(s->key.reserve((size_t)H));
        CAND_HIP(s->key_sorted.reserve((size_t)H));
        CAND_HIP(s->flag.reserve((size_t)H));
        CAND_HIP(s->pos.reserve((size_t)H));
        hipLaunchKernelGGL(k_cand_hits<true>, dim3(gn), dim3(BLOCK), 0, st, t->view(), s->al.p, n, s->cnt.p, (const u64*)s->off.p, s->key.p, H);
        // (2) visiting order
        const int key_bits = 32 + bits_for(n);
        CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortKeys(w, wb, s->key.p, s->key_sorted.p, (int)H, 0, key_bits, st);
        }));
        hipLaunchKernelGGL(k_heads, dim3(gh), dim3(BLOCK), 0, st, (const u64*)s->key_sorted.p, H, s->flag.p);
        CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, s->flag.p, s->pos.p, (int)H, st); }));
        if (const int rc = flag_total(st, s->flag.p, s->pos.p, H, &V)) return rc;
        if (V < 1 || V > H) return CAND_FAIL(DSA_E_DEVICE, "internal: %lld distinct of %lld overlaps", (long long)V, (long long)H);
        const unsigned gv = grid_of(V);
        CAND_HIP(s->vkey.reserve((size_t)V));
        CAND_HIP(s->ckey.reserve((size_t)V));
        CAND_HIP(s->ckey_sorted.reserve((size_t)V));
        CAND_HIP(s->rank.reserve((size_t)V));
        CAND_HIP(s->rank_sorted.reserve((size_t)V));
        CAND_HIP(s->keep_v.reserve((size_t)V));
        CAND_HIP(s->keep_s.reserve((size_t)V));
        CAND_HIP(s->kpos.reserve((size_t)V));
        hipLaunchKernelGGL(k_cand_visit, dim3(gh), dim3(BLOCK), 0, st, (const u64*)s->key_sorted.p, s->flag.p, s->pos.p, H, V, s->al.p, s->vkey.p, s->ckey.p,
                           s->rank.p);
        // (3) first come, first kept: the stable sort leaves the first-visited of equal keys at the head of its run
        CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, s->ckey.p, s->ckey_sorted.p, s->rank.p, s->rank_sorted.p, (int)V, 0, 64, st);
        }));
        hipLaunchKernelGGL(k_cand_keep, dim3(gv), dim3(BLOCK), 0, st, (const u64*)s->ckey_sorted.p, s->rank_sorted.p, V, (const u64*)s->seen.p, s->n_seen,
                           s->keep_v.p, s->keep_s.p);
        CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, s->keep_v.p, s->kpos.p, (int)V, st); }));
        if (const int rc = flag_total(st, s->keep_v.p, s->kpos.p, V, &K)) return rc;
        if (K < 0 || K > V) return CAND_FAIL(DSA_E_DEVICE, "internal: %lld kept of %lld visited", (long long)K, (long long)V);
    }
    *n_out = K;
    if (timing) { timing->n_hits = H; timing->n_visited = V; timing->n_kept = K; }
    if (!RESIDENT && K > cap) return CAND_FAIL(DSA_E_CAPACITY, "%lld candidates, room for %lld", (long long)K, (long long)cap);   // the session is as it was

    if (K) {
        const unsigned gv = grid_of(V), gk = grid_of(K);
        // (4) records
        CAND_HIP(s->rec.reserve((size_t)K));
        CAND_HIP(s->fkey.reserve((size_t)K));
        CAND_HIP(s->idx.reserve((size_t)K));
        hipLaunchKernelGGL(k_cand_emit, dim3(gv), dim3(BLOCK), 0, st, (const u64*)s->vkey.p, (const u64*)s->ckey.p, s->keep_v.p, s->kpos.p, V, K, s->given, s->rec.p);
        hipLaunchKernelGGL(k_cand_first, dim3(gk), dim3(BLOCK), 0, st, s->rec.p, K, s->fkey.p, s->idx.p);
        const cand_record* result = s->rec.p;
        if (order == CAND_ORDER_FUSION) {
            CAND_HIP(s->rec_sorted.reserve((size_t)K));
            CAND_HIP(s->fkey_sorted.reserve((size_t)K));
            CAND_HIP(s->idx_sorted.reserve((size_t)K));
            CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) {
                return hipcub::DeviceRadixSort::SortPairs(w, wb, s->fkey.p, s->fkey_sorted.p, s->idx.p, s->idx_sorted.p, (int)K, 0, 31, st);
            }));
            hipLaunchKernelGGL(k_cand_gather, dim3(gk), dim3(BLOCK), 0, st, (const cand_record*)s->rec.p, s->idx_sorted.p, K, s->rec_sorted.p);
            result = s->rec_sorted.p;
        }
        // (5) the new seen keys into a second array; the session takes it over when the records are on the host
        CAND_HIP(s->new_keys.reserve((size_t)K));
        CAND_HIP(s->seen_next.reserve((size_t)(s->n_seen + K)));
        CAND_HIP(hiphost::cub_run(s->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, s->keep_s.p, s->kpos.p, (int)V, st); }));
        hipLaunchKernelGGL(k_cand_newkeys, dim3(gv), dim3(BLOCK), 0, st, (const u64*)s->ckey_sorted.p, s->keep_s.p, s->kpos.p, V, K, s->new_keys.p);
        hipLaunchKernelGGL(k_cand_merge, dim3(grid_of(s->n_seen + K)), dim3(BLOCK), 0, st, (const u64*)s->seen.p, s->n_seen, (const u64*)s->new_keys.p, K,
                           s->seen_next.p);
        CAND_HIP(hipEventRecord(s->ev[2], st));
        if (!RESIDENT) CAND_HIP(hipMemcpyAsync(out, result, (size_t)K * sizeof(cand_record), hipMemcpyDeviceToHost, st));
        CAND_HIP(hipEventRecord(s->ev[3], st));
        if (RESIDENT) {
            s->resident = result;
            s->n_resident = K;
        }
    } else {
        CAND_HIP(hipEventRecord(s->ev[2], st));
        CAND_HIP(hipEventRecord(s->ev[3], st));
    }
    CAND_HIP(hipStreamSynchronize(st));
    CAND_HIP(hipGetLastError());
    if (K) {
        s->seen.swap(s->seen_next);
        s->n_seen += K;
    }
    s->given += n;
    if (timing) {
        timing->upload_ms = hiphost::elapsed(s->ev[0], s->ev[1]);
        timing->device_ms = hiphost::elapsed(s->ev[1], s->ev[2]);
        timing->download_ms = RESIDENT ? 0.f : hiphost::elapsed(s->ev[2], s->ev[3]);
    }
    return DSA_OK;
}

}  // namespace

extern "C" {

int cand_enumerate(cand_session* s, const cand_alignment* alignments, int64_t n, int32_t order, cand_record* out, int64_t cap,
                   int64_t* n_out, cand_timing* timing)
{
    return enumerate<false>(s, alignments, n, order, out, cap, n_out, timing);
}

int cand_enumerate_device(cand_session* s, const cand_alignment* alignments, int64_t n, int32_t order, int64_t* n_out, cand_timing* timing)
{
    return enumerate<true>(s, alignments, n, order, nullptr, 0, n_out, timing);
}

int cand_enumerate_resident(cand_session* s, const void* alignments_device, int64_t n, int32_t order, int64_t* n_out, int64_t* first_bad, cand_timing* timing)
{
    if (!first_bad) return CAND_FAIL(DSA_E_ARG, "cand_enumerate_resident: no first_bad");
    return enumerate<true, true>(s, static_cast<const cand_alignment*>(alignments_device), n, order, nullptr, 0, n_out, timing, first_bad);
}

int cand_records_device(const cand_session* s, const void** dev, int64_t* n)
{
    if (!s || !dev || !n) return CAND_FAIL(DSA_E_ARG, "cand_records_device: no %s", !s ? "session" : "output");
    *dev = s->resident;
    *n = s->n_resident;
    return DSA_OK;
}

}  // extern "C"
