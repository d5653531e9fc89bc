// eval_api.hip — SplitAlignmentTask::Evaluate (tools/SplitAlignment.cpp:484-594) for all groups of a batch on gfx950
// (include/defuse_eval.h): per run of equal fusion ids the refSplit with the largest summed score, its support, the kept
// records and the two FP64 statistics.
//
// Device pipeline, n records; the host waits once for the group count (the grid of the last kernel) and once for the results:
//   k_eval_columns   the 40-byte records -> columns (refSplit, readSplit, score) and a flag where a group begins
//   InclusiveSum     flags -> dense group id + 1 per record; k_eval_group_start notes where each group begins
//   two stable radix sorts of the record indices: by ref_second, then by (group id, ref_first), both coordinates XORed with
//                    2^31 so that unsigned order is signed order.  A group occupies the same index range before and after.
//   k_eval_run_in    marks runs of equal (group, split) in that order; a segmented inclusive scan sums score (64 bits) and
//                    counts records per run, complete at a run's last record
//   k_eval_best_in   + a segmented scan over the groups that keeps the FIRST run with the largest sum: ascending split order
//                    and "first" are the std::map walk with the strict '>' of the reference.  Complete at a group's last
//                    record, where k_eval_group writes the group's row.
//   k_eval_keep      in INPUT order: records at their group's best split; ExclusiveSum + k_eval_compact list their indices
//   k_eval_stats     one wavefront per group: 64 kept records at a time, each lane forms the two quotients of its record, then
//                    every lane adds the 64 terms serially in record order (shuffles), so a group's sum is one chain of IEEE
//                    additions however large the group is.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <string>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_eval.h"
#include "hip_host.hpp"
#include "pred_shared.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::grid_of;

thread_local std::string g_eval_err;

#define EVAL_HIP(call) HIPHOST_TRY(g_eval_err, call)

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr uint32_t BIAS = 0x80000000u;
constexpr int MIN_ANCHOR = 4;          // tools/SplitAlignment.cpp:29

static_assert(sizeof(dsa_record) == 40 && sizeof(eval_group) == 72 && sizeof(eval_timing) == 56, "C ABI layout");

// what the host reads back once the kernels are done
struct Counts {
    uint32_t n_groups, n_kept, n_runs, n_flagged, overflow;
};

// per-run sum of score and record count: a head starts a new run
struct RunSum {
    long long sum;
    uint32_t cnt;
    uint32_t head;
};
struct RunSumOp {
    __host__ __device__ RunSum operator()(const RunSum& a, const RunSum& b) const
    {
        return b.head ? b : RunSum{a.sum + b.sum, a.cnt + b.cnt, a.head};
    }
};

// the first run with the largest sum of a group: pos = sorted position of the run's last record; only such records carry a
// candidate (VALID), the others are the identity inside their group
constexpr uint32_t B_HEAD = 1, B_VALID = 2;
struct Best {
    long long sum;
    uint32_t pos;
    uint32_t flags;
};
struct BestOp {
    __host__ __device__ Best operator()(const Best& a, const Best& b) const
    {
        if (b.flags & B_HEAD) return b;
        Best r = !(a.flags & B_VALID) ? b : !(b.flags & B_VALID) ? a : (b.sum > a.sum ? b : a);
        r.flags = ((a.flags | b.flags) & B_VALID) | (a.flags & B_HEAD);
        return r;
    }
};

__global__ void k_eval_columns(const int32_t* __restrict__ rec, int64_t n, int32_t* __restrict__ rf, int32_t* __restrict__ rs,
                               int32_t* __restrict__ qf, int32_t* __restrict__ qs, int32_t* __restrict__ score, uint32_t* __restrict__ ghead)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t* r = rec + i * 10;                                // dsa_record: ten ints, 8-byte aligned
    const int2 ref = *reinterpret_cast<const int2*>(r + 4);
    const int2 read = *reinterpret_cast<const int2*>(r + 6);
    rf[i] = ref.x; rs[i] = ref.y;
    qf[i] = read.x; qs[i] = read.y;
    score[i] = r[8];
    ghead[i] = (i == 0 || r[0] != r[-10]) ? 1u : 0u;
}

__global__ void k_eval_group_start(const uint32_t* __restrict__ ghead, const uint32_t* __restrict__ gid1, int64_t n, uint32_t* __restrict__ gstart,
                                   uint32_t* __restrict__ key1, const int32_t* __restrict__ rs, uint32_t* __restrict__ idx, Counts* __restrict__ c)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (ghead[i]) gstart[gid1[i] - 1] = (uint32_t)i;
    key1[i] = (uint32_t)rs[i] ^ BIAS;
    idx[i] = (uint32_t)i;
    if (i == n - 1) c->n_groups = gid1[i];
}

__global__ void k_eval_key2(const uint32_t* __restrict__ idx1, const uint32_t* __restrict__ gid1, const int32_t* __restrict__ rf, int64_t n,
                            unsigned long long* __restrict__ key2)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx1[j];
    key2[j] = ((unsigned long long)(gid1[i] - 1) << 32) | (unsigned long long)((uint32_t)rf[i] ^ BIAS);
}

// sorted order: ref_second beside the key, and the run scan's input
__global__ void k_eval_run_in(const unsigned long long* __restrict__ key2, const uint32_t* __restrict__ sidx, const int32_t* __restrict__ rs,
                              const int32_t* __restrict__ score, int64_t n, int32_t* __restrict__ rs_sorted, RunSum* __restrict__ out,
                              Counts* __restrict__ c)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = sidx[j];
    const int32_t s = rs[i];
    rs_sorted[j] = s;
    const bool head = j == 0 || key2[j] != key2[j - 1] || s != rs[sidx[j - 1]];
    out[j] = RunSum{(long long)score[i], 1u, head ? 1u : 0u};
    const unsigned long long heads = __ballot(head);                // one add per wavefront: the count is for eval_timing only
    if (head && (int)(threadIdx.x % WAVE) == __ffsll((long long)heads) - 1) atomicAdd(&c->n_runs, (uint32_t)__popcll(heads));
}

__global__ void k_eval_best_in(const unsigned long long* __restrict__ key2, const RunSum* __restrict__ run_in, const RunSum* __restrict__ run, int64_t n,
                               Best* __restrict__ out, Counts* __restrict__ c)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const bool ghead = j == 0 || (key2[j] >> 32) != (key2[j - 1] >> 32);
    const bool last = j + 1 == n || run_in[j + 1].head != 0;       // the run's sum is complete here
    const long long sum = run[j].sum;
    if (last && (sum > (long long)INT_MAX || sum < (long long)INT_MIN)) c->overflow = 1u;
    out[j] = Best{sum, (uint32_t)j, (ghead ? B_HEAD : 0u) | (last ? B_VALID : 0u)};
}

// at the last record of a group (sorted order): its row but for the kept offset and the statistics
__global__ void k_eval_group(const int32_t* __restrict__ rec, const unsigned long long* __restrict__ key2, const int32_t* __restrict__ rs_sorted,
                             const RunSum* __restrict__ run, const Best* __restrict__ best, const uint32_t* __restrict__ gstart, int64_t n,
                             eval_group* __restrict__ groups)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t g = (uint32_t)(key2[j] >> 32);
    if (j + 1 < n && (uint32_t)(key2[j + 1] >> 32) == g) return;
    const Best b = best[j];
    const uint32_t first = gstart[g];
    eval_group o{};
    o.fusion_id = rec[(int64_t)first * 10];
    o.first_record = first;
    o.n_records = j + 1 - (int64_t)first;
    if (b.sum > -1) {                                               // maxScore starts at -1, strict '>' (:506-516)
        o.best_first = (int32_t)((uint32_t)key2[b.pos] ^ BIAS);
        o.best_second = rs_sorted[b.pos];
        o.best_score = (int32_t)b.sum;                              // (in range, or the call fails)
        o.count = run[b.pos].cnt;
    } else {
        o.status = EVAL_NO_SPLIT;
    }
    groups[g] = o;
}

// input order; keep[n] = 0 so that the exclusive sum's last entry is the count
__global__ void k_eval_keep(const uint32_t* __restrict__ gid1, const int32_t* __restrict__ rf, const int32_t* __restrict__ rs,
                            const eval_group* __restrict__ groups, int64_t n, uint32_t* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i > n) return;
    uint32_t k = 0;
    if (i < n) {
        const eval_group* g = groups + (gid1[i] - 1);
        k = (!(g->status & EVAL_NO_SPLIT) && rf[i] == g->best_first && rs[i] == g->best_second) ? 1u : 0u;
    }
    keep[i] = k;
}

__global__ void k_eval_compact(const uint32_t* __restrict__ ghead, const uint32_t* __restrict__ gid1, const uint32_t* __restrict__ keep,
                               const uint32_t* __restrict__ koff, int64_t n, int64_t* __restrict__ kept, eval_group* __restrict__ groups,
                               Counts* __restrict__ c)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (keep[i]) kept[koff[i]] = i;
    if (ghead[i]) groups[gid1[i] - 1].kept_off = koff[i];
    if (i == n - 1) c->n_kept = koff[n];
}

// one wavefront per group (file comment).  No contraction: quotient and sum are separate IEEE operations.
__global__ void __launch_bounds__(BLOCK) k_eval_stats(const int64_t* __restrict__ kept, const int32_t* __restrict__ qf, const int32_t* __restrict__ qs,
                                                      uint32_t n_groups, eval_group* __restrict__ groups, Counts* __restrict__ c)
{
#pragma clang fp contract(off)
    const uint32_t g = (uint32_t)(((int64_t)blockIdx.x * BLOCK + threadIdx.x) / WAVE);
    const int lane = threadIdx.x % WAVE;
    if (g >= n_groups) return;                                      // (whole wavefronts leave)
    eval_group* out = groups + g;
    if (out->status & EVAL_NO_SPLIT) return;
    const int64_t off = out->kept_off, cnt = out->count;
    double pos_sum = 0.0, min_sum = 0.0;
    bool flagged = false;
    for (int64_t base = 0; base < cnt; base += WAVE) {
        const int m = (int)(cnt - base < WAVE ? cnt - base : WAVE);
        double pq = 0.0, mq = 0.0;
        bool bad = false;
        if (lane < m) {
            const int64_t i = kept[off + base + lane];
            const int left = qf[i], right = qs[i];
            const long long range = (long long)left + (long long)right - 2 * MIN_ANCHOR;
            bad = range <= 1;
            const double posRange = (double)range;
            const double posValue = (double)(left - MIN_ANCHOR > 0 ? (long long)left - MIN_ANCHOR : 0);
            const double minRange = floor(0.5 * (double)range);
            const long long lo = left < right ? (long long)left - MIN_ANCHOR : (long long)right - MIN_ANCHOR;
            const double minValue = (double)(lo > 0 ? lo : 0);
            if (!bad) {
                pq = posValue / posRange;
                mq = minValue / minRange;
            }
        }
        flagged |= __any(bad) != 0;
        for (int t = 0; t < m; ++t) {                               // m is the same in every lane: all lanes add the same chain
            pos_sum += __shfl(pq, t, WAVE);
            min_sum += __shfl(mq, t, WAVE);
        }
    }
    if (lane == 0) {
        if (flagged) {
            out->status |= EVAL_HOST_STATS;
            atomicAdd(&c->n_flagged, 1u);
        } else {
            out->pos_sum = pos_sum;
            out->min_sum = min_sum;
        }
    }
}

}  // namespace

struct eval_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[5];
    eval_timing timing{};
    int64_t resident_groups = -1;                                   // groups[0 .. resident_groups) are the latest successful call's; -1: none
    DeviceBuffer<int32_t, hiphost::GrowSize> rec;                   // the host entry's copy of the records (ten ints each)
    DeviceBuffer<int32_t, hiphost::GrowSize> rf, rs, qf, qs, score, rs_sorted;
    DeviceBuffer<uint32_t, hiphost::GrowSize> ghead, gid1, gstart, key1, key1_sorted, idx0, idx1, sidx, keep, koff;
    DeviceBuffer<unsigned long long, hiphost::GrowSize> key2, key2_sorted;
    DeviceBuffer<RunSum, hiphost::GrowSize> run_in, run;
    DeviceBuffer<Best, hiphost::GrowSize> best_in, best;
    DeviceBuffer<eval_group, hiphost::GrowSize> groups;
    DeviceBuffer<int64_t, hiphost::GrowSize> kept;
    DeviceBuffer<Counts> counts;
    DeviceBuffer<uint8_t, hiphost::GrowSize> tmp;
};

namespace {

int eval_reserve(eval_ctx* c, size_t n)
{
    EVAL_HIP(c->rf.reserve(n));
    EVAL_HIP(c->rs.reserve(n));
    EVAL_HIP(c->qf.reserve(n));
    EVAL_HIP(c->qs.reserve(n));
    EVAL_HIP(c->score.reserve(n));
    EVAL_HIP(c->rs_sorted.reserve(n));
    EVAL_HIP(c->ghead.reserve(n));
    EVAL_HIP(c->gid1.reserve(n));
    EVAL_HIP(c->gstart.reserve(n));
    EVAL_HIP(c->key1.reserve(n));
    EVAL_HIP(c->key1_sorted.reserve(n));
    EVAL_HIP(c->idx0.reserve(n));
    EVAL_HIP(c->idx1.reserve(n));
    EVAL_HIP(c->sidx.reserve(n));
    EVAL_HIP(c->keep.reserve(n + 1));
    EVAL_HIP(c->koff.reserve(n + 1));
    EVAL_HIP(c->key2.reserve(n));
    EVAL_HIP(c->key2_sorted.reserve(n));
    EVAL_HIP(c->run_in.reserve(n));
    EVAL_HIP(c->run.reserve(n));
    EVAL_HIP(c->best_in.reserve(n));
    EVAL_HIP(c->best.reserve(n));
    EVAL_HIP(c->groups.reserve(n));
    EVAL_HIP(c->kept.reserve(n));
    EVAL_HIP(c->counts.reserve(1));
    return DSA_OK;
}

// records: host memory (on_device false) or memory of the ctx's device
int eval_run(eval_ctx* c, const void* records, bool on_device, int64_t n, eval_group* groups, int64_t group_cap, int64_t* n_groups,
             int64_t* kept, int64_t kept_cap, int64_t* n_kept)
{
    if (!c || n < 0 || (n && !records) || !n_groups || !n_kept || group_cap < 0 || kept_cap < 0) {
        g_eval_err = "eval_groups: null pointer or negative count";
        if (c) c->resident_groups = -1;
        return DSA_E_ARG;
    }
    c->resident_groups = -1;                                        // until this call has succeeded
    *n_groups = *n_kept = 0;
    // 32-bit scans, slots and sort counts
    if (n >= INT32_MAX - 1) { g_eval_err = "more than 2^31 - 2 records in one call"; return DSA_E_LIMIT; }
    c->timing = eval_timing{};
    if (n == 0) {
        c->resident_groups = 0;
        return DSA_OK;
    }
    EVAL_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int rc = eval_reserve(c, (size_t)n);
    if (rc != DSA_OK) return rc;
    const int32_t* rec = (const int32_t*)records;
    EVAL_HIP(hipEventRecord(c->ev[0], st));
    if (!on_device) {
        EVAL_HIP(c->rec.reserve((size_t)n * 10));
        EVAL_HIP(hipMemcpyAsync(c->rec.p, records, (size_t)n * sizeof(dsa_record), hipMemcpyHostToDevice, st));
        rec = c->rec.p;
    }
    EVAL_HIP(hipEventRecord(c->ev[1], st));
    EVAL_HIP(hipMemsetAsync(c->counts.p, 0, sizeof(Counts), st));
    const unsigned g = grid_of(n), g1 = grid_of(n + 1);
    const int ni = (int)n;
    int gid_bits = 1;
    while (gid_bits < 31 && ((int64_t)1 << gid_bits) < n) ++gid_bits;           // group ids are below n
    hipLaunchKernelGGL(k_eval_columns, dim3(g), dim3(BLOCK), 0, st, rec, n, c->rf.p, c->rs.p, c->qf.p, c->qs.p, c->score.p, c->ghead.p);
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::InclusiveSum(t, tb, c->ghead.p, c->gid1.p, ni, st);
    }));
    hipLaunchKernelGGL(k_eval_group_start, dim3(g), dim3(BLOCK), 0, st, c->ghead.p, c->gid1.p, n, c->gstart.p, c->key1.p, c->rs.p, c->idx0.p,
                       c->counts.p);
    // stable, least significant key first: equal (group, split) keep the input order
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceRadixSort::SortPairs(t, tb, c->key1.p, c->key1_sorted.p, c->idx0.p, c->idx1.p, ni, 0, 32, st);
    }));
    hipLaunchKernelGGL(k_eval_key2, dim3(g), dim3(BLOCK), 0, st, c->idx1.p, c->gid1.p, c->rf.p, n, c->key2.p);
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceRadixSort::SortPairs(t, tb, c->key2.p, c->key2_sorted.p, c->idx1.p, c->sidx.p, ni, 0, 32 + gid_bits, st);
    }));
    const unsigned long long* K = c->key2_sorted.p;
    hipLaunchKernelGGL(k_eval_run_in, dim3(g), dim3(BLOCK), 0, st, K, c->sidx.p, c->rs.p, c->score.p, n, c->rs_sorted.p, c->run_in.p, c->counts.p);
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::InclusiveScan(t, tb, c->run_in.p, c->run.p, RunSumOp(), ni, st);
    }));
    hipLaunchKernelGGL(k_eval_best_in, dim3(g), dim3(BLOCK), 0, st, K, c->run_in.p, c->run.p, n, c->best_in.p, c->counts.p);
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::InclusiveScan(t, tb, c->best_in.p, c->best.p, BestOp(), ni, st);
    }));
    hipLaunchKernelGGL(k_eval_group, dim3(g), dim3(BLOCK), 0, st, rec, K, c->rs_sorted.p, c->run.p, c->best.p, c->gstart.p, n, c->groups.p);
    hipLaunchKernelGGL(k_eval_keep, dim3(g1), dim3(BLOCK), 0, st, c->gid1.p, c->rf.p, c->rs.p, c->groups.p, n, c->keep.p);
    EVAL_HIP(hiphost::cub_run(c->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::ExclusiveSum(t, tb, c->keep.p, c->koff.p, ni + 1, st);
    }));
    hipLaunchKernelGGL(k_eval_compact, dim3(g), dim3(BLOCK), 0, st, c->ghead.p, c->gid1.p, c->keep.p, c->koff.p, n, c->kept.p, c->groups.p,
                       c->counts.p);
    // the statistics kernel takes one wavefront per group: its grid needs the group count
    Counts cnt{};
    EVAL_HIP(hipMemcpyAsync(&cnt, c->counts.p, sizeof(Counts), hipMemcpyDeviceToHost, st));
    EVAL_HIP(hipStreamSynchronize(st));
    if (cnt.n_groups == 0 || (int64_t)cnt.n_groups > n || (int64_t)cnt.n_kept > n) { g_eval_err = "internal: group or kept count out of range"; return DSA_E_DEVICE; }
    hipLaunchKernelGGL(k_eval_stats, dim3(grid_of((int64_t)cnt.n_groups * WAVE)), dim3(BLOCK), 0, st, c->kept.p, c->qf.p, c->qs.p, cnt.n_groups,
                       c->groups.p, c->counts.p);
    EVAL_HIP(hipEventRecord(c->ev[2], st));
    EVAL_HIP(hipMemcpyAsync(&cnt, c->counts.p, sizeof(Counts), hipMemcpyDeviceToHost, st));
    EVAL_HIP(hipStreamSynchronize(st));
    EVAL_HIP(hipGetLastError());
    c->timing.upload_ms = on_device ? 0.f : hiphost::elapsed(c->ev[0], c->ev[1]);      // nothing is copied for records on the device
    c->timing.device_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.n_records = n;
    c->timing.n_groups = cnt.n_groups;
    c->timing.n_runs = cnt.n_runs;
    c->timing.n_kept = cnt.n_kept;
    c->timing.n_flagged = cnt.n_flagged;
    if (cnt.overflow) {
        g_eval_err = "the summed score of a split leaves the int32 range (the reference's int overflows there)";
        return DSA_E_LIMIT;
    }
    *n_groups = cnt.n_groups;
    *n_kept = cnt.n_kept;
    if ((int64_t)cnt.n_groups > group_cap || (int64_t)cnt.n_kept > kept_cap) {
        g_eval_err = "eval_groups: " + std::to_string(cnt.n_groups) + " groups and " + std::to_string(cnt.n_kept) + " kept records do not fit the capacities";
        return DSA_E_CAPACITY;
    }
    if (!groups || (cnt.n_kept && !kept)) { g_eval_err = "eval_groups: null output pointer"; return DSA_E_ARG; }
    EVAL_HIP(hipEventRecord(c->ev[3], st));
    EVAL_HIP(hipMemcpyAsync(groups, c->groups.p, (size_t)cnt.n_groups * sizeof(eval_group), hipMemcpyDeviceToHost, st));
    if (cnt.n_kept) EVAL_HIP(hipMemcpyAsync(kept, c->kept.p, (size_t)cnt.n_kept * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    EVAL_HIP(hipEventRecord(c->ev[4], st));
    EVAL_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    c->resident_groups = cnt.n_groups;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* eval_last_error(void) { return g_eval_err.c_str(); }

int eval_create(int device, eval_ctx** out)
{
    if (!out) { g_eval_err = "eval_create: null pointer"; return DSA_E_ARG; }
    *out = nullptr;
    if (hiphost::check_device(device, &g_eval_err)) return DSA_E_DEVICE;
    EVAL_HIP(hipSetDevice(device));
    eval_ctx* c = new eval_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        g_eval_err = "cannot create a stream";
        return DSA_E_DEVICE;
    }
    *out = c;
    return DSA_OK;
}

void eval_destroy(eval_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int eval_groups(eval_ctx* c, const dsa_record* records, int64_t n, eval_group* groups, int64_t group_cap, int64_t* n_groups, int64_t* kept,
                int64_t kept_cap, int64_t* n_kept)
{
    return eval_run(c, records, false, n, groups, group_cap, n_groups, kept, kept_cap, n_kept);
}

int eval_groups_device(eval_ctx* c, const void* records_device, int64_t n, eval_group* groups, int64_t group_cap, int64_t* n_groups, int64_t* kept,
                       int64_t kept_cap, int64_t* n_kept)
{
    return eval_run(c, records_device, true, n, groups, group_cap, n_groups, kept, kept_cap, n_kept);
}

// include/defuse_pred.h; here because it reads the ctx.  The groups are complete: eval_run has synchronised its stream.
int pred_predict_resident(pred_ctx* ctx, const pred_tasks* tasks, const eval_ctx* eval)
{
    if (!ctx || !tasks || !eval) return predint::fail(DSA_E_ARG, "pred_predict_resident: no %s", !ctx ? "ctx" : !tasks ? "tasks" : "eval ctx");
    if (eval->resident_groups < 0) {
        predint::clear(ctx);
        return predint::fail(DSA_E_ARG, "pred_predict_resident: the eval ctx has no completed evaluation (none yet, or its latest call failed or was refused)");
    }
    return predint::predict_device("pred_predict_resident", ctx, tasks, eval->groups.p, eval->resident_groups, eval->device);
}

int eval_get_timing(const eval_ctx* c, eval_timing* out)
{
    if (!c || !out) { g_eval_err = "eval_get_timing: null pointer"; return DSA_E_ARG; }
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
