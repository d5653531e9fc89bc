// bat_api.hip — the batch assembly between the candidate loop and the split-read DP on gfx950 (include/defuse_bat.h):
// mReads[readID.id], ReverseComplement and the task lookup of SplitReadRealigner::DoAlignment (tools/SplitAlignment.cpp:
// 286-294) for all kept candidates of a call at once.  The result is a dsa batch (ref_bytes, fusions, read_bytes, pairs) in
// device buffers, byte for byte what defuse_amd/cand.py:dsa_batch builds on the host.
//
// Reads (bat_reads_create).  Key = ReadID.id as an unsigned word; one STABLE radix sort of (key, record index) puts the last
// given of equal keys at the tail of its run, a tail-flag compaction keeps it: distinct keys ascending with offset and length.
// Windows (bat_windows_create).  The host has to look at every fusion_id anyway to refuse a double one, so the windows go up
// sorted by fusion_id; the position in that order is the window's slot.
//
// Assembly (bat_assemble*), all on the batch's stream, one host round trip:
//   (1) lookup: one thread per candidate finds its read and its window slot by binary search; atomicMin leaves the first
//       candidate position of every slot, and the lowest record whose fusion_id has no windows;
//   (2) a 64-bit exclusive sum of the read lengths gives read_off; flags of the used slots are summed, their window lengths
//       reduced; the totals come back in one small copy and are tested before the byte buffers are sized;
//   (3) the used slots are compacted and sorted by first position (a radix sort of distinct keys: deterministic), which is
//       the order of fusions[]; an exclusive sum of their window lengths gives the ref offsets;
//   (4) pairs, fusions and one 16-byte segment descriptor per read and per window are written;
//   (5) the gather (k_bat_gather) copies the segments, reads reversed and complemented where revcomp is set.
//
// The gather kernel, its segment record and the window store's struct are in bat_shared.hpp (pred_api.hip uses them too).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "../../include/defuse_bat.h"
#include "../../include/defuse_text.h"     // bat_reads_create_device
#include "bat_shared.hpp"
#include "hip_host.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using batdev::Seg;
using batdev::SRC_PAD;
using batdev::WindowsView;
using u64 = unsigned long long;

thread_local std::string g_bat_err;

#define BAT_HIP(call) HIPHOST_TRY(g_bat_err, call)
#define BAT_FAIL(code, ...) hiphost::fail(g_bat_err, code, __VA_ARGS__)

constexpr int BLOCK = batdev::GATHER_BLOCK;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int READ_GROUP = 16;        // lanes per read: 150 bases are 38 dwords, three steps of 16
constexpr int WINDOW_GROUP = 64;      // lanes per window: a few hundred bases and more

__host__ __device__ inline uint32_t read_key(int32_t fragment, int32_t read_end)
{
    return ((uint32_t)fragment & 0x7FFFFFFFu) | ((uint32_t)(read_end & 1) << 31);
}

// the first index in [0, n) with a[index] >= x
__device__ inline int64_t lower_bound(const uint32_t* __restrict__ a, int64_t n, uint32_t x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- reads ------------------------------------------------------------------------------------------------------------

__global__ void k_reads_keys(const bat_read* __restrict__ rec, int64_t n, uint32_t* __restrict__ key, uint32_t* __restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    key[i] = read_key(rec[i].fragment, rec[i].read_end);
    idx[i] = (uint32_t)i;
}

// the last of a run of equal keys is the read that was given last (the sort is stable)
__global__ void k_reads_tails(const uint32_t* __restrict__ key, int64_t n, uint32_t* __restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == n - 1 || key[i] != key[i + 1]) ? 1u : 0u;
}

__global__ void k_reads_unique(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ flag,
                               const uint32_t* __restrict__ pos, int64_t n, int64_t n_unique, const bat_read* __restrict__ rec,
                               uint32_t* __restrict__ ukey, int64_t* __restrict__ uoff, int32_t* __restrict__ ulen)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || !flag[i] || (int64_t)pos[i] >= n_unique || (int64_t)idx[i] >= n) return;
    const bat_read r = rec[idx[i]];
    ukey[pos[i]] = key[i];
    uoff[pos[i]] = r.off;
    ulen[pos[i]] = r.len;
}

// bat_reads_create's per-record checks for records that are on the device: the lowest bad one
__global__ void k_reads_check(const bat_read* __restrict__ rec, int64_t n, int64_t bytes_len, uint32_t* __restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const bat_read r = rec[i];
    if (r.fragment < 0 || (r.read_end != 0 && r.read_end != 1) || r.len < 0 || r.off < 0 || r.off > bytes_len || (int64_t)r.len > bytes_len - r.off)
        atomicMin(bad, (uint32_t)i);
}

struct ReadsView {
    const uint32_t* ukey;       // n_unique distinct ReadID.id, ascending as unsigned
    const int64_t* uoff;
    const int32_t* ulen;
    int64_t n_unique;
};

// ---- assembly ---------------------------------------------------------------------------------------------------------

struct Totals {
    u64 read_total;             // bytes of read_bytes
    u64 ref_total;              // bytes of ref_bytes
    uint32_t bad;               // lowest record whose fusion_id has no windows, NONE if there is none
    uint32_t n_used;            // fusions of the batch
};

__global__ void k_bat_lookup(const cand_record* __restrict__ cand, int64_t n, ReadsView r, WindowsView w, u64* __restrict__ rlen,
                             uint32_t* __restrict__ ridx, uint32_t* __restrict__ slot, uint32_t* __restrict__ first, Totals* __restrict__ tot)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const cand_record c = cand[k];
    const uint32_t key = read_key(c.fragment, c.read_end);
    const int64_t p = lower_bound(r.ukey, r.n_unique, key);
    const bool have = p < r.n_unique && r.ukey[p] == key;
    ridx[k] = have ? (uint32_t)p : NONE;
    rlen[k] = have ? (u64)r.ulen[p] : 0;
    const int64_t s = lower_bound(w.wkey, w.n, (uint32_t)c.fusion_id);
    if (s < w.n && w.wkey[s] == (uint32_t)c.fusion_id) {
        slot[k] = (uint32_t)s;
        atomicMin(&first[s], (uint32_t)k);
    } else {
        slot[k] = NONE;
        atomicMin(&tot->bad, (uint32_t)k);
    }
}

__global__ void k_bat_slots(const uint32_t* __restrict__ first, WindowsView w, uint32_t* __restrict__ flag, u64* __restrict__ wlen)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= w.n) return;
    const bool used = first[s] != NONE;
    flag[s] = used ? 1u : 0u;
    wlen[s] = used ? (u64)w.wfus[s].ref0_len + (u64)w.wfus[s].ref1_len : 0;
}

// one thread: the totals next to ref_total (written by the reduction) and bad (by the lookup)
__global__ void k_bat_totals(const u64* __restrict__ rlen, const u64* __restrict__ roff, int64_t n, const uint32_t* __restrict__ flag,
                             const uint32_t* __restrict__ upos, int64_t n_windows, Totals* __restrict__ tot)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    tot->read_total = roff[n - 1] + rlen[n - 1];
    tot->n_used = upos[n_windows - 1] + flag[n_windows - 1];
}

__global__ void k_bat_compact(const uint32_t* __restrict__ first, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ upos,
                              int64_t n_windows, int64_t n_used, uint32_t* __restrict__ ckey, uint32_t* __restrict__ cslot)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= n_windows || !flag[s] || (int64_t)upos[s] >= n_used) return;
    ckey[upos[s]] = first[s];
    cslot[upos[s]] = (uint32_t)s;
}

// in the order of first appearance: fusion j is slot order[j]
__global__ void k_bat_order(const uint32_t* __restrict__ order, int64_t n_used, WindowsView w, u64* __restrict__ wlen, uint32_t* __restrict__ fidx_of_slot)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_used || (int64_t)order[j] >= w.n) return;
    const dsa_fusion f = w.wfus[order[j]];
    wlen[j] = (u64)f.ref0_len + (u64)f.ref1_len;
    fidx_of_slot[order[j]] = (uint32_t)j;
}

__global__ void k_bat_fusions(const uint32_t* __restrict__ order, const u64* __restrict__ woff, int64_t n_used, WindowsView w,
                              dsa_fusion* __restrict__ fusions, Seg* __restrict__ seg)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_used || (int64_t)order[j] >= w.n) return;
    const dsa_fusion f = w.wfus[order[j]];
    const int32_t o = (int32_t)woff[j];
    fusions[j] = dsa_fusion{f.fusion_id, o, f.ref0_len, o + f.ref0_len, f.ref1_len};
    seg[2 * j] = Seg{(int64_t)f.ref0_off, o, (uint32_t)f.ref0_len};
    seg[2 * j + 1] = Seg{(int64_t)f.ref1_off, o + f.ref0_len, (uint32_t)f.ref1_len};
}

__global__ void k_bat_pairs(const cand_record* __restrict__ cand, int64_t n, ReadsView r, const u64* __restrict__ rlen, const u64* __restrict__ roff,
                            const uint32_t* __restrict__ ridx, const uint32_t* __restrict__ slot, const uint32_t* __restrict__ fidx_of_slot,
                            int64_t n_windows, dsa_pair* __restrict__ pairs, Seg* __restrict__ seg)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const cand_record c = cand[k];
    const uint32_t len = (uint32_t)rlen[k];
    dsa_pair p;
    p.fusion_idx = (int64_t)slot[k] < n_windows ? (int32_t)fidx_of_slot[slot[k]] : -1;      // (every slot is known here: the host has seen bad == NONE)
    p.read_off = (int32_t)roff[k];
    p.read_len = (int32_t)len;
    p.frag = c.fragment;
    p.read_end = c.read_end;
    p.revcomp = c.revcomp;
    p.pad_[0] = p.pad_[1] = 0;
    pairs[k] = p;
    const bool have = (int64_t)ridx[k] < r.n_unique;
    seg[k] = Seg{have ? r.uoff[ridx[k]] : 0, p.read_off, (have ? len : 0u) | (c.revcomp ? 0x80000000u : 0u)};
}

int bits_for(int64_t n)      // bits that hold 0 .. n - 1, at least one
{
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < n) ++b;
    return b;
}

}  // namespace

struct bat_reads {
    int device = -1;
    int64_t n_unique = 0, bytes_len = 0;
    hiphost::Stream st;
    DeviceBuffer<uint8_t> bytes;
    DeviceBuffer<uint32_t> ukey;
    DeviceBuffer<int64_t> uoff;
    DeviceBuffer<int32_t> ulen;
    ReadsView view() const { return ReadsView{ukey.p, uoff.p, ulen.p, n_unique}; }
};

struct bat_batch {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[5];        // 0 start, 1 candidates uploaded, 2 lookup done, 3 descriptors done, 4 gathers done
    // the batch
    int64_t n_pairs = 0, read_bytes_len = 0, ref_bytes_len = 0;
    int32_t n_fusions = 0;
    DeviceBuffer<uint8_t, GrowSize> ref_bytes, read_bytes;
    DeviceBuffer<dsa_fusion, GrowSize> fusions;
    DeviceBuffer<dsa_pair, GrowSize> pairs;
    // per call
    DeviceBuffer<cand_record, GrowSize> cands;
    DeviceBuffer<u64, GrowSize> rlen, roff, wlen, woff;
    DeviceBuffer<uint32_t, GrowSize> ridx, slot, first, flag, upos, ckey, ckey_sorted, cslot, order, fidx_of_slot;
    DeviceBuffer<Seg, GrowSize> seg_reads, seg_windows;
    DeviceBuffer<Totals, GrowSize> totals;
    DeviceBuffer<uint8_t, GrowSize> tmp;
    bat_timing timing{};
};

namespace {

// why bat_reads_create refuses a record, "" if it does not
std::string read_fault(const bat_read& r, long long k, int64_t bytes_len)
{
    char buf[160] = "";
    if (r.fragment < 0) snprintf(buf, sizeof buf, "read %lld: fragment %d is outside [0, 2^31)", k, r.fragment);
    else if (r.read_end != 0 && r.read_end != 1) snprintf(buf, sizeof buf, "read %lld: read_end %d is not 0 or 1", k, r.read_end);
    else if (r.len < 0) snprintf(buf, sizeof buf, "read %lld: negative length %d", k, r.len);
    else if (r.off < 0 || r.off > bytes_len || (int64_t)r.len > bytes_len - r.off)
        snprintf(buf, sizeof buf, "read %lld: bytes %lld + %d are outside the %lld given", k, (long long)r.off, r.len, (long long)bytes_len);
    return buf;
}

// DEVICE: bytes and reads are device pointers of the store's GPU, and the records are checked here, by a kernel
template <bool DEVICE>
int reads_build(bat_reads* r, const uint8_t* bytes, const bat_read* reads, int64_t n)
{
    hipStream_t st = r->st;
    const hipMemcpyKind kind = DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    BAT_HIP(r->bytes.reserve((size_t)r->bytes_len + SRC_PAD));
    BAT_HIP(r->ukey.reserve(1));
    BAT_HIP(r->uoff.reserve(1));
    BAT_HIP(r->ulen.reserve(1));
    if (r->bytes_len) BAT_HIP(hipMemcpyAsync(r->bytes.p, bytes, (size_t)r->bytes_len, kind, st));
    if (n == 0) {
        BAT_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    }
    DeviceBuffer<bat_read> rec;
    DeviceBuffer<uint32_t> key, key_sorted, idx, idx_sorted, flag, pos;
    DeviceBuffer<uint8_t> tmp;
    BAT_HIP(rec.reserve((size_t)n));
    BAT_HIP(key.reserve((size_t)n));
    BAT_HIP(key_sorted.reserve((size_t)n));
    BAT_HIP(idx.reserve((size_t)n));
    BAT_HIP(idx_sorted.reserve((size_t)n));
    BAT_HIP(flag.reserve((size_t)n));
    BAT_HIP(pos.reserve((size_t)n));
    BAT_HIP(hipMemcpyAsync(rec.p, reads, (size_t)n * sizeof(bat_read), kind, st));
    if (DEVICE) {
        uint32_t bad = NONE;
        BAT_HIP(hipMemcpyAsync(flag.p, &bad, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_reads_check, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const bat_read*)rec.p, n, r->bytes_len, flag.p);
        BAT_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        BAT_HIP(hipStreamSynchronize(st));
        BAT_HIP(hipGetLastError());
        if (bad != NONE) {
            if ((int64_t)bad >= n) return BAT_FAIL(DSA_E_DEVICE, "internal: bad read %u of %lld", bad, (long long)n);
            bat_read one{};
            BAT_HIP(hipMemcpy(&one, rec.p + bad, sizeof(bat_read), hipMemcpyDeviceToHost));
            return BAT_FAIL(DSA_E_ARG, "%s", read_fault(one, (long long)bad, r->bytes_len).c_str());
        }
    }
    hipLaunchKernelGGL(k_reads_keys, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const bat_read*)rec.p, n, key.p, idx.p);
    // stable: of equal keys the last given stays last
    BAT_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, key.p, key_sorted.p, idx.p, idx_sorted.p, (int)n, 0, 32, st);
    }));
    hipLaunchKernelGGL(k_reads_tails, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const uint32_t*)key_sorted.p, n, flag.p);
    BAT_HIP(hiphost::cub_run(tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, flag.p, pos.p, (int)n, st); }));
    uint32_t last[2] = {0, 0};
    BAT_HIP(hipMemcpyAsync(&last[0], pos.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BAT_HIP(hipMemcpyAsync(&last[1], flag.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    BAT_HIP(hipStreamSynchronize(st));
    const int64_t U = (int64_t)last[0] + (int64_t)last[1];
    if (U < 1 || U > n) return BAT_FAIL(DSA_E_DEVICE, "internal: %lld distinct keys of %lld reads", (long long)U, (long long)n);
    BAT_HIP(r->ukey.reserve((size_t)U));
    BAT_HIP(r->uoff.reserve((size_t)U));
    BAT_HIP(r->ulen.reserve((size_t)U));
    hipLaunchKernelGGL(k_reads_unique, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const uint32_t*)key_sorted.p, (const uint32_t*)idx_sorted.p,
                       (const uint32_t*)flag.p, (const uint32_t*)pos.p, n, U, (const bat_read*)rec.p, r->ukey.p, r->uoff.p, r->ulen.p);
    BAT_HIP(hipStreamSynchronize(st));
    BAT_HIP(hipGetLastError());
    r->n_unique = U;
    return DSA_OK;
}

// the store object around reads_build, after the argument checks
template <bool DEVICE>
int reads_create(int device, const uint8_t* bytes, int64_t bytes_len, const bat_read* reads, int64_t n, bat_reads** out)
{
    if (hiphost::check_device(device, &g_bat_err)) return DSA_E_DEVICE;
    BAT_HIP(hipSetDevice(device));
    bat_reads* r = new bat_reads();
    r->device = device;
    r->bytes_len = bytes_len;
    int rc = DSA_OK;
    if (r->st.create(hipStreamNonBlocking) != hipSuccess) rc = BAT_FAIL(DSA_E_DEVICE, "cannot create a stream");
    if (rc == DSA_OK) rc = reads_build<DEVICE>(r, bytes, reads, n);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(r->st);
        delete r;
        return rc;
    }
    *out = r;
    return DSA_OK;
}

// everything after the candidates are on the device (b->ev[1] recorded)
int assemble_on_device(bat_reads* reads, bat_windows* windows, const cand_record* cand, int64_t n, bat_batch* b)
{
    hipStream_t st = b->st;
    const int64_t W = windows->n;
    const ReadsView rv = reads->view();
    const WindowsView wv = windows->view();
    const unsigned gn = grid_of(n), gw = grid_of(W);

    BAT_HIP(b->rlen.reserve((size_t)n));
    BAT_HIP(b->roff.reserve((size_t)n));
    BAT_HIP(b->ridx.reserve((size_t)n));
    BAT_HIP(b->slot.reserve((size_t)n));
    BAT_HIP(b->first.reserve((size_t)W));
    BAT_HIP(b->flag.reserve((size_t)W));
    BAT_HIP(b->upos.reserve((size_t)W));
    BAT_HIP(b->wlen.reserve((size_t)W));
    BAT_HIP(b->woff.reserve((size_t)W));
    BAT_HIP(b->fidx_of_slot.reserve((size_t)W));
    BAT_HIP(b->totals.reserve(1));

    // (1) lookup
    const Totals init{0, 0, NONE, 0};
    BAT_HIP(hipMemcpyAsync(b->totals.p, &init, sizeof(Totals), hipMemcpyHostToDevice, st));
    BAT_HIP(hipMemsetAsync(b->first.p, 0xFF, (size_t)W * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_bat_lookup, dim3(gn), dim3(BLOCK), 0, st, cand, n, rv, wv, b->rlen.p, b->ridx.p, b->slot.p, b->first.p, b->totals.p);
    BAT_HIP(hipEventRecord(b->ev[2], st));
    // (2) sums; every total in 64 bits
    BAT_HIP(hiphost::cub_run(b->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, b->rlen.p, b->roff.p, (int)n, st); }));
    hipLaunchKernelGGL(k_bat_slots, dim3(gw), dim3(BLOCK), 0, st, (const uint32_t*)b->first.p, wv, b->flag.p, b->wlen.p);
    BAT_HIP(hiphost::cub_run(b->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, b->flag.p, b->upos.p, (int)W, st); }));
    BAT_HIP(hiphost::cub_run(b->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceReduce::Sum(w, wb, b->wlen.p, &b->totals.p->ref_total, (int)W, st); }));
    hipLaunchKernelGGL(k_bat_totals, dim3(1), dim3(64), 0, st, (const u64*)b->rlen.p, (const u64*)b->roff.p, n, (const uint32_t*)b->flag.p,
                       (const uint32_t*)b->upos.p, W, b->totals.p);
    Totals tot{};
    BAT_HIP(hipMemcpyAsync(&tot, b->totals.p, sizeof(Totals), hipMemcpyDeviceToHost, st));
    BAT_HIP(hipStreamSynchronize(st));
    BAT_HIP(hipGetLastError());
    if (tot.bad != NONE) return BAT_FAIL(DSA_E_ARG, "record %u: fusion_id has no windows", tot.bad);
    if (tot.read_total > (u64)INT32_MAX)
        return BAT_FAIL(DSA_E_LIMIT, "%llu read bytes in one batch: more than 2^31 - 1, give fewer candidates per call", tot.read_total);
    if (tot.ref_total > (u64)INT32_MAX)
        return BAT_FAIL(DSA_E_LIMIT, "%llu window bytes in one batch: more than 2^31 - 1, give fewer candidates per call", tot.ref_total);
    const int64_t U = (int64_t)tot.n_used, RB = (int64_t)tot.read_total, WB = (int64_t)tot.ref_total;
    if (U < 1 || U > W || U > n) return BAT_FAIL(DSA_E_DEVICE, "internal: %lld fusions of %lld candidates and %lld windows", (long long)U, (long long)n, (long long)W);

    // (3) the used fusions in the order of their first candidates
    const unsigned gu = grid_of(U);
    BAT_HIP(b->ckey.reserve((size_t)U));
    BAT_HIP(b->ckey_sorted.reserve((size_t)U));
    BAT_HIP(b->cslot.reserve((size_t)U));
    BAT_HIP(b->order.reserve((size_t)U));
    BAT_HIP(b->seg_reads.reserve((size_t)n));
    BAT_HIP(b->seg_windows.reserve((size_t)(2 * U)));
    BAT_HIP(b->pairs.reserve((size_t)n));
    BAT_HIP(b->fusions.reserve((size_t)U));
    BAT_HIP(b->read_bytes.reserve((size_t)RB + 4));          // whole dwords
    BAT_HIP(b->ref_bytes.reserve((size_t)WB + 4));
    hipLaunchKernelGGL(k_bat_compact, dim3(gw), dim3(BLOCK), 0, st, (const uint32_t*)b->first.p, (const uint32_t*)b->flag.p, (const uint32_t*)b->upos.p, W, U,
                       b->ckey.p, b->cslot.p);
    BAT_HIP(hiphost::cub_run(b->tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, b->ckey.p, b->ckey_sorted.p, b->cslot.p, b->order.p, (int)U, 0, bits_for(n), st);
    }));
    // (wlen is free again: the reduction over the slots is done)
    hipLaunchKernelGGL(k_bat_order, dim3(gu), dim3(BLOCK), 0, st, (const uint32_t*)b->order.p, U, wv, b->wlen.p, b->fidx_of_slot.p);
    BAT_HIP(hiphost::cub_run(b->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, b->wlen.p, b->woff.p, (int)U, st); }));
    // (4) descriptors
    hipLaunchKernelGGL(k_bat_fusions, dim3(gu), dim3(BLOCK), 0, st, (const uint32_t*)b->order.p, (const u64*)b->woff.p, U, wv, b->fusions.p, b->seg_windows.p);
    hipLaunchKernelGGL(k_bat_pairs, dim3(gn), dim3(BLOCK), 0, st, cand, n, rv, (const u64*)b->rlen.p, (const u64*)b->roff.p, (const uint32_t*)b->ridx.p,
                       (const uint32_t*)b->slot.p, (const uint32_t*)b->fidx_of_slot.p, W, b->pairs.p, b->seg_reads.p);
    BAT_HIP(hipEventRecord(b->ev[3], st));
    // (5) the gathers
    hipLaunchKernelGGL(k_bat_gather<READ_GROUP>, dim3(grid_of(n * READ_GROUP)), dim3(BLOCK), 0, st, (const Seg*)b->seg_reads.p, n,
                       (const uint8_t*)reads->bytes.p, reads->bytes_len, b->read_bytes.p, RB);
    hipLaunchKernelGGL(k_bat_gather<WINDOW_GROUP>, dim3(grid_of(2 * U * WINDOW_GROUP)), dim3(BLOCK), 0, st, (const Seg*)b->seg_windows.p, 2 * U,
                       (const uint8_t*)windows->bytes.p, windows->bytes_len, b->ref_bytes.p, WB);
    BAT_HIP(hipEventRecord(b->ev[4], st));
    BAT_HIP(hipStreamSynchronize(st));
    BAT_HIP(hipGetLastError());
    b->n_pairs = n;
    b->n_fusions = (int32_t)U;
    b->read_bytes_len = RB;
    b->ref_bytes_len = WB;
    b->timing.lookup_ms = hiphost::elapsed(b->ev[1], b->ev[2]);
    b->timing.scan_ms = hiphost::elapsed(b->ev[2], b->ev[3]);
    b->timing.gather_ms = hiphost::elapsed(b->ev[3], b->ev[4]);
    b->timing.n_fusions = U;
    b->timing.read_bytes = RB;
    b->timing.ref_bytes = WB;
    return DSA_OK;
}

int assemble(const char* what, bat_reads* reads, bat_windows* windows, const void* cands, bool on_device, int64_t n, bat_batch* b)
{
    if (!reads || !windows || !b) return BAT_FAIL(DSA_E_ARG, "%s: no %s", what, !reads ? "reads" : !windows ? "windows" : "batch");
    if (n < 0) return BAT_FAIL(DSA_E_ARG, "negative number of candidates (%lld)", (long long)n);
    if (n > (int64_t)INT32_MAX) return BAT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 candidates in one call");
    if (n && !cands) return BAT_FAIL(DSA_E_ARG, "%s: no candidates", what);
    if (reads->device != windows->device || reads->device != b->device)
        return BAT_FAIL(DSA_E_ARG, "%s: reads, windows and batch are on devices %d, %d and %d", what, reads->device, windows->device, b->device);
    b->n_pairs = b->read_bytes_len = b->ref_bytes_len = 0;
    b->n_fusions = 0;
    b->timing = bat_timing{0, 0, 0, 0, n, 0, 0, 0};
    BAT_HIP(hipSetDevice(b->device));
    // the view of an empty batch has pointers too
    BAT_HIP(b->pairs.reserve(1));
    BAT_HIP(b->fusions.reserve(1));
    BAT_HIP(b->read_bytes.reserve(4));
    BAT_HIP(b->ref_bytes.reserve(4));
    if (n == 0) return DSA_OK;
    if (windows->n == 0) return BAT_FAIL(DSA_E_ARG, "record 0: fusion_id has no windows");
    hipStream_t st = b->st;
    const cand_record* dev = static_cast<const cand_record*>(cands);
    BAT_HIP(hipEventRecord(b->ev[0], st));
    if (!on_device) {
        BAT_HIP(b->cands.reserve((size_t)n));
        BAT_HIP(hipMemcpyAsync(b->cands.p, cands, (size_t)n * sizeof(cand_record), hipMemcpyHostToDevice, st));
        dev = b->cands.p;
    }
    BAT_HIP(hipEventRecord(b->ev[1], st));
    const int rc = assemble_on_device(reads, windows, dev, n, b);
    if (rc == DSA_OK && !on_device) b->timing.upload_ms = hiphost::elapsed(b->ev[0], b->ev[1]);
    if (rc != DSA_OK) (void)hipStreamSynchronize(st);          // nothing of a refused call is in flight when it returns
    return rc;
}

}  // namespace

extern "C" {

const char* bat_last_error(void) { return g_bat_err.c_str(); }

int bat_reads_create(int device, const uint8_t* bytes, int64_t bytes_len, const bat_read* reads, int64_t n, bat_reads** out)
{
    if (!out) return BAT_FAIL(DSA_E_ARG, "bat_reads_create: no output");
    *out = nullptr;
    if (n < 0 || bytes_len < 0) return BAT_FAIL(DSA_E_ARG, "negative size (%lld reads, %lld bytes)", (long long)n, (long long)bytes_len);
    if (n > (int64_t)INT32_MAX) return BAT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 reads in one store");
    if ((n && !reads) || (bytes_len && !bytes)) return BAT_FAIL(DSA_E_ARG, "bat_reads_create: null pointer with non-zero size");
    for (int64_t k = 0; k < n; ++k) {
        const std::string fault = read_fault(reads[k], (long long)k, bytes_len);
        if (!fault.empty()) return BAT_FAIL(DSA_E_ARG, "%s", fault.c_str());
    }
    return reads_create<false>(device, bytes, bytes_len, reads, n, out);
}

int bat_reads_create_device(int device, const void* bytes_device, int64_t bytes_len, const void* reads_device, int64_t n, bat_reads** out)
{
    if (!out) return BAT_FAIL(DSA_E_ARG, "bat_reads_create_device: no output");
    *out = nullptr;
    if (n < 0 || bytes_len < 0) return BAT_FAIL(DSA_E_ARG, "negative size (%lld reads, %lld bytes)", (long long)n, (long long)bytes_len);
    if (n > (int64_t)INT32_MAX) return BAT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 reads in one store");
    if ((n && !reads_device) || (bytes_len && !bytes_device)) return BAT_FAIL(DSA_E_ARG, "bat_reads_create_device: null pointer with non-zero size");
    return reads_create<true>(device, static_cast<const uint8_t*>(bytes_device), bytes_len, static_cast<const bat_read*>(reads_device), n, out);
}

void bat_reads_destroy(bat_reads* r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->st);
    delete r;
}

int bat_windows_create(int device, const uint8_t* ref_bytes, int64_t ref_bytes_len, const dsa_fusion* fusions, int32_t n, bat_windows** out)
{
    if (!out) return BAT_FAIL(DSA_E_ARG, "bat_windows_create: no output");
    *out = nullptr;
    if (n < 0 || ref_bytes_len < 0) return BAT_FAIL(DSA_E_ARG, "negative size (%d fusions, %lld bytes)", n, (long long)ref_bytes_len);
    if (ref_bytes_len > (int64_t)INT32_MAX) return BAT_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 window bytes in one store");
    if ((n && !fusions) || (ref_bytes_len && !ref_bytes)) return BAT_FAIL(DSA_E_ARG, "bat_windows_create: null pointer with non-zero size");
    dsa_limits lim{};
    (void)dsa_get_limits(nullptr, &lim);
    std::vector<std::pair<uint32_t, int32_t>> byid((size_t)n);
    for (int32_t f = 0; f < n; ++f) {
        const dsa_fusion& fu = fusions[f];
        if (fu.ref0_len < 0 || fu.ref1_len < 0 || fu.ref0_off < 0 || fu.ref1_off < 0 || (int64_t)fu.ref0_off + fu.ref0_len > ref_bytes_len ||
            (int64_t)fu.ref1_off + fu.ref1_len > ref_bytes_len)
            return BAT_FAIL(DSA_E_ARG, "fusion %d: reference window outside ref_bytes", f);
        if (fu.ref0_len > lim.max_ref_len || fu.ref1_len > lim.max_ref_len)
            return BAT_FAIL(DSA_E_LIMIT, "fusion %d: reference window longer than %d", f, lim.max_ref_len);
        byid[(size_t)f] = {(uint32_t)fu.fusion_id, f};
    }
    std::sort(byid.begin(), byid.end());
    for (int32_t s = 1; s < n; ++s)
        if (byid[(size_t)s].first == byid[(size_t)s - 1].first)
            return BAT_FAIL(DSA_E_ARG, "fusions %d and %d: both have fusion_id %d", byid[(size_t)s - 1].second, byid[(size_t)s].second,
                            (int32_t)byid[(size_t)s].first);
    if (hiphost::check_device(device, &g_bat_err)) return DSA_E_DEVICE;
    BAT_HIP(hipSetDevice(device));
    std::vector<uint32_t> wkey((size_t)n);
    std::vector<dsa_fusion> wfus((size_t)n);
    for (int32_t s = 0; s < n; ++s) {
        wkey[(size_t)s] = byid[(size_t)s].first;
        wfus[(size_t)s] = fusions[byid[(size_t)s].second];
    }
    bat_windows* w = new bat_windows();
    w->device = device;
    w->n = n;
    w->bytes_len = ref_bytes_len;
    auto build = [&]() -> int {
        if (w->st.create(hipStreamNonBlocking) != hipSuccess) return BAT_FAIL(DSA_E_DEVICE, "cannot create a stream");
        hipStream_t st = w->st;
        BAT_HIP(w->bytes.reserve((size_t)ref_bytes_len + SRC_PAD));
        BAT_HIP(w->wkey.reserve((size_t)n));
        BAT_HIP(w->wfus.reserve((size_t)n));
        if (ref_bytes_len) BAT_HIP(hipMemcpyAsync(w->bytes.p, ref_bytes, (size_t)ref_bytes_len, hipMemcpyHostToDevice, st));
        if (n) BAT_HIP(hipMemcpyAsync(w->wkey.p, wkey.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (n) BAT_HIP(hipMemcpyAsync(w->wfus.p, wfus.data(), (size_t)n * sizeof(dsa_fusion), hipMemcpyHostToDevice, st));
        BAT_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    };
    if (const int rc = build()) {
        (void)hipStreamSynchronize(w->st);
        delete w;
        return rc;
    }
    *out = w;
    return DSA_OK;
}

void bat_windows_destroy(bat_windows* w)
{
    if (!w) return;
    (void)hipSetDevice(w->device);
    (void)hipStreamSynchronize(w->st);
    delete w;
}

int bat_batch_create(int device, bat_batch** out)
{
    if (!out) return BAT_FAIL(DSA_E_ARG, "bat_batch_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_bat_err)) return DSA_E_DEVICE;
    BAT_HIP(hipSetDevice(device));
    bat_batch* b = new bat_batch();
    b->device = device;
    bool ok = b->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : b->ev) ok = ok && e.create() == hipSuccess;
    ok = ok && b->pairs.reserve(1) == hipSuccess && b->fusions.reserve(1) == hipSuccess && b->read_bytes.reserve(4) == hipSuccess &&
         b->ref_bytes.reserve(4) == hipSuccess;
    if (!ok) {
        delete b;
        return BAT_FAIL(DSA_E_DEVICE, "cannot create a stream or a buffer");
    }
    *out = b;
    return DSA_OK;
}

void bat_batch_destroy(bat_batch* b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->st);
    delete b;
}

int bat_assemble(bat_reads* reads, bat_windows* windows, const cand_record* cands, int64_t n, bat_batch* batch)
{
    return assemble("bat_assemble", reads, windows, cands, false, n, batch);
}

int bat_assemble_device(bat_reads* reads, bat_windows* windows, const void* cands_device, int64_t n, bat_batch* batch)
{
    return assemble("bat_assemble_device", reads, windows, cands_device, true, n, batch);
}

int bat_batch_view(const bat_batch* b, bat_view* out)
{
    if (!b || !out) return BAT_FAIL(DSA_E_ARG, "bat_batch_view: no %s", !b ? "batch" : "output");
    *out = bat_view{b->ref_bytes.p, b->fusions.p, b->read_bytes.p, b->pairs.p, b->ref_bytes_len, b->read_bytes_len, b->n_pairs, b->n_fusions, b->device};
    return DSA_OK;
}

int bat_batch_fetch(bat_batch* b, uint8_t* ref_bytes, int64_t ref_cap, dsa_fusion* fusions, int64_t fusions_cap, uint8_t* read_bytes, int64_t read_cap,
                    dsa_pair* pairs, int64_t pairs_cap)
{
    if (!b) return BAT_FAIL(DSA_E_ARG, "bat_batch_fetch: no batch");
    if (ref_cap < 0 || fusions_cap < 0 || read_cap < 0 || pairs_cap < 0) return BAT_FAIL(DSA_E_ARG, "bat_batch_fetch: negative capacity");
    if ((ref_cap && !ref_bytes) || (fusions_cap && !fusions) || (read_cap && !read_bytes) || (pairs_cap && !pairs))
        return BAT_FAIL(DSA_E_ARG, "bat_batch_fetch: capacity without a buffer");
    if (ref_cap < b->ref_bytes_len || fusions_cap < b->n_fusions || read_cap < b->read_bytes_len || pairs_cap < b->n_pairs)
        return BAT_FAIL(DSA_E_CAPACITY, "the batch has %lld ref bytes, %d fusions, %lld read bytes, %lld pairs", (long long)b->ref_bytes_len, b->n_fusions,
                        (long long)b->read_bytes_len, (long long)b->n_pairs);
    BAT_HIP(hipSetDevice(b->device));
    hipStream_t st = b->st;
    if (b->ref_bytes_len) BAT_HIP(hipMemcpyAsync(ref_bytes, b->ref_bytes.p, (size_t)b->ref_bytes_len, hipMemcpyDeviceToHost, st));
    if (b->n_fusions) BAT_HIP(hipMemcpyAsync(fusions, b->fusions.p, (size_t)b->n_fusions * sizeof(dsa_fusion), hipMemcpyDeviceToHost, st));
    if (b->read_bytes_len) BAT_HIP(hipMemcpyAsync(read_bytes, b->read_bytes.p, (size_t)b->read_bytes_len, hipMemcpyDeviceToHost, st));
    if (b->n_pairs) BAT_HIP(hipMemcpyAsync(pairs, b->pairs.p, (size_t)b->n_pairs * sizeof(dsa_pair), hipMemcpyDeviceToHost, st));
    BAT_HIP(hipStreamSynchronize(st));
    return DSA_OK;
}

int bat_get_timing(const bat_batch* b, bat_timing* out)
{
    if (!b || !out) return BAT_FAIL(DSA_E_ARG, "bat_get_timing: no %s", !b ? "batch" : "output");
    *out = b->timing;
    return DSA_OK;
}

}  // extern "C"
