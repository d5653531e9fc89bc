// cmpp_api.hip — the EM problems of clustermatepairs built on gfx950 from the bin pairs (include/defuse_cmp.h,
// cmp_problems_*): the stages tools_src/clustermatepairs.cpp runs on host threads between cmp_bin_run and mpe_cluster_batch
// (the reference's tools/clustermatepairs.cpp:292-375,478-545), and the choice of the lines to print (:549-583).
//
// Every step is a grid of independent threads, a hipcub scan, run-length encode or STABLE radix sort; no atomics, no
// order that depends on the launch shape.  In the order they run (s = side, 0 `first` / 1 `second`):
//   candidates      flag per bin pair, scan, compaction                       -> cand_k[c], ccoff[s][c] (entries of candidates)
//   grouping        key (c << 32 | fragment as ordered uint32) per entry, stable sort, run-length encode
//                                                                              -> groups (c, fragment) with their entries in list order
//   matching        binary search of every group's key among the other side's groups
//   filter          one lane per matched group walks its entries in list order and links the kept ones into a chain
//                   (the chain lives in the entries' own link[] slots: no per-lane array, any group length)
//   problems        matched groups per candidate from a scan; survivors numbered by a scan
//   mate pairs      per group |kept first| x |kept second|, 64-bit scan; one thread per mate pair fills pairs, x, y, u
//   ranks           key (problem << 32 | x descending), stable sort: the position inside the problem is the rank
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defuse_cmp.h"
#include "../../include/defuse_dsa.h"
#include "cmp_shared.hpp"
#include "hip_host.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::grid_of;
typedef unsigned long long u64;

using cmpshared::cmp_err;

#define CMP_HIP(call) HIPHOST_TRY(cmp_err(), call)

constexpr int BIN_LENGTH = 1 << 15;            // tools/clustermatepairs.cpp:385 (binLength)

// the lists of all bin pairs on the device, wherever they live (the binner's buffers, or this object's uploads)
struct Lists {
    const u64* keys;
    const int* off[2];
    const cmp_packed* pay[2];
};

// signed order of the fragment as unsigned order of the result
__device__ inline uint32_t ordered(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

// first index in [0, n) whose element is >= v (n if none)
template <typename T>
__device__ inline int64_t lower_bound(const T* a, int64_t n, T v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// last index in [0, n) whose element is <= v: a[] are ascending offsets with a[0] <= v
template <typename T>
__device__ inline int64_t owner_of(const T* a, int64_t n, T v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

struct Align { int ref, strand, fragment, read_end, start, end; };
// the unpacked alignment (tools_src/clustermatepairs.cpp:629-640): id = RefBinPacked of the side, region relative to its bin
__device__ inline Align unpack(uint32_t id, const cmp_packed& p)
{
    const int bin = (int)(id >> 19);
    Align a;
    a.ref = (int)(id & 0x3FFFFu);
    a.strand = (int)((id >> 18) & 1u);
    a.fragment = p.fragment;
    a.read_end = p.read_end;
    a.start = (int)p.rel_start + bin * BIN_LENGTH - BIN_LENGTH / 2;
    a.end = (int)p.rel_end + bin * BIN_LENGTH - BIN_LENGTH / 2;
    return a;
}
__device__ inline uint32_t side_id(u64 key, int s) { return s == 0 ? (uint32_t)(key >> 32) : (uint32_t)(key & 0xFFFFFFFFu); }

__global__ void k_candidates(Lists L, int64_t nk, int mcs, int* __restrict__ flag)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nk) return;
    // (int)size < minClusterSize skips the bin pair (:627)
    flag[k] = k < nk && L.off[0][k + 1] - L.off[0][k] >= mcs && L.off[1][k + 1] - L.off[1][k] >= mcs;
}

__global__ void k_compact_candidates(Lists L, int64_t nk, const int* __restrict__ flag, const int* __restrict__ cidx, int64_t nc,
                                     int* __restrict__ cand_k, int* __restrict__ clen0, int* __restrict__ clen1)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) clen0[nc] = clen1[nc] = 0;             // one more element: the scans' last output is the total
    if (k >= nk || !flag[k]) return;
    const int c = cidx[k];
    cand_k[c] = (int)k;
    clen0[c] = L.off[0][k + 1] - L.off[0][k];
    clen1[c] = L.off[1][k + 1] - L.off[1][k];
}

// entry i of the candidates' entries of one side: its sort key (candidate, fragment) and itself as the value
__global__ void k_entry_keys(const cmp_packed* __restrict__ pay, const int* __restrict__ off, const int* __restrict__ cand_k,
                             const int* __restrict__ ccoff, int64_t nc, int64_t m, u64* __restrict__ key, uint32_t* __restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t c = owner_of(ccoff, nc + 1, (int)i);
    const cmp_packed& p = pay[off[cand_k[c]] + ((int)i - ccoff[c])];
    key[i] = ((u64)c << 32) | ordered(p.fragment);
    val[i] = (uint32_t)i;
}

// FilterUnmatched: the group of the same (candidate, fragment) on the other side, -1 if there is none
__global__ void k_match(const u64* __restrict__ gkey, int64_t ng, const u64* __restrict__ other, int64_t ng_other, int* __restrict__ partner)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int64_t at = lower_bound(other, ng_other, gkey[g]);
    partner[g] = at < ng_other && other[at] == gkey[g] ? (int)at : -1;
}

// FilterOverlapping (:316-358), one lane per group of one side.  All alignments of a list share (reference, strand), so a
// bin is taken iff an alignment kept before, of the same read end, covers it.  link[j] of a sorted entry: -1 dropped, else
// 1 + the group-relative position of the previous kept entry of the group (0: none) — the chain of the kept ones, walked
// backwards.  Kept ranges of one read end are disjoint, so the chain is as long as the distinct bins allow, not the group.
__global__ void k_filter(Lists L, int s, int mfr, const int* __restrict__ cand_k, const int* __restrict__ ccoff,
                         const u64* __restrict__ gkey, const int* __restrict__ gstart, const int* __restrict__ partner, int64_t ng,
                         const uint32_t* __restrict__ sidx, int* __restrict__ link, int* __restrict__ kept)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const int j0 = gstart[g], j1 = gstart[g + 1];
    if (partner[g] < 0) {
        for (int j = j0; j < j1; ++j) { link[j] = -1; kept[j] = 0; }
        return;
    }
    const int c = (int)(gkey[g] >> 32), k = cand_k[c];
    const int bin = (int)(side_id(L.keys[k], s) >> 19);
    const cmp_packed* pay = L.pay[s] + L.off[s][k] - ccoff[c];            // indexed by the entry's number among the candidates' entries
    int last = 0;                                                           // 1 + position of the last kept entry
    for (int j = j0; j < j1; ++j) {
        const cmp_packed p = pay[sidx[j]];
        const int start = (int)p.rel_start + bin * BIN_LENGTH - BIN_LENGTH / 2, end = (int)p.rel_end + bin * BIN_LENGTH - BIN_LENGTH / 2;
        const int sb = start / mfr, eb = end / mfr;                         // GetBins with extend 0: C++ division, towards zero
        bool overlapping = false;
        if (sb <= eb)                                                       // (an empty range takes no bin and meets none)
            for (int q = last; q > 0 && !overlapping; q = link[j0 + q - 1]) {
                const cmp_packed o = pay[sidx[j0 + q - 1]];
                if (o.read_end != p.read_end) continue;
                const int os = ((int)o.rel_start + bin * BIN_LENGTH - BIN_LENGTH / 2) / mfr, oe = ((int)o.rel_end + bin * BIN_LENGTH - BIN_LENGTH / 2) / mfr;
                overlapping = os <= oe && sb <= oe && os <= eb;
            }
        if (overlapping) { link[j] = -1; kept[j] = 0; }
        else { link[j] = last; kept[j] = 1; last = j - j0 + 1; }
    }
}

__global__ void k_kept_list(const int* __restrict__ kept, const int* __restrict__ kpos, int64_t m, int* __restrict__ klist)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m && kept[j]) klist[kpos[j]] = (int)j;
}

__global__ void k_matched_flags(const int* __restrict__ partner, int64_t ng, int* __restrict__ matched)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= ng) matched[g] = g < ng && partner[g] >= 0;
}

// a candidate survives with at least min_cluster_size matched fragments (:648; both sides hold the same ones)
__global__ void k_survivors(const u64* __restrict__ gkey0, int64_t ng0, const int* __restrict__ mpre, int64_t nc, int mcs,
                            int* __restrict__ glo, int* __restrict__ surv)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nc) return;
    if (c == nc) { surv[c] = 0; return; }
    const int64_t lo = lower_bound(gkey0, ng0, (u64)c << 32), hi = lower_bound(gkey0, ng0, (u64)(c + 1) << 32);
    glo[c] = (int)lo;
    surv[c] = mpre[hi] - mpre[lo] >= mcs;
}

// GetAlignPairs (:360-375): a matched fragment of a problem gives |kept first| x |kept second| mate pairs
__global__ void k_pair_counts(const u64* __restrict__ gkey0, const int* __restrict__ partner0, int64_t ng0, const int* __restrict__ surv,
                              const int* __restrict__ gstart0, const int* __restrict__ kpos0, const int* __restrict__ gstart1,
                              const int* __restrict__ kpos1, long long* __restrict__ pcnt)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > ng0) return;
    long long n = 0;
    if (g < ng0 && partner0[g] >= 0 && surv[gkey0[g] >> 32]) {
        const int g1 = partner0[g];
        n = (long long)(kpos0[gstart0[g + 1]] - kpos0[gstart0[g]]) * (long long)(kpos1[gstart1[g1 + 1]] - kpos1[gstart1[g1]]);
    }
    pcnt[g] = n;
}

__global__ void k_problem_table(const int* __restrict__ surv, const int* __restrict__ pidx, const int* __restrict__ glo, const int* __restrict__ cand_k,
                                const long long* __restrict__ poff, int64_t nc, int64_t ng0, int64_t np, long long* __restrict__ prob_off,
                                int32_t* __restrict__ prob_bin, int32_t* __restrict__ prob_group)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) { prob_off[np] = poff[ng0]; prob_group[np] = (int32_t)ng0; }
    if (c >= nc || !surv[c]) return;
    const int p = pidx[c];
    prob_off[p] = poff[glo[c]];
    prob_bin[p] = cand_k[c];
    prob_group[p] = glo[c];
}

__device__ inline void strand_remap(const Align& a, int& start, int& end)      // tools/MatePairEM.cpp:75-83
{
    start = a.strand == 0 ? a.start : -a.end;
    end = a.strand == 0 ? a.end : -a.start;
}

struct GroupTables {
    const u64* gkey0;
    const int *partner0, *gstart[2], *kpos[2], *klist[2], *ccoff[2];
    const uint32_t* sidx[2];
    const int *cand_k, *pidx;
    const long long* poff;
    int64_t ng0;
};

// mate pair i: its fragment group from the 64-bit offsets, its two alignments from the position inside the product
__global__ __launch_bounds__(256) void k_mate_pairs(Lists L, GroupTables T, int64_t n_mp, double fragment_mean, cmp_pair* __restrict__ pairs,
                                                     double* __restrict__ x, double* __restrict__ y, double* __restrict__ u,
                                                     u64* __restrict__ xkey, u64* __restrict__ ykey, uint32_t* __restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mp) return;
    const int64_t g = owner_of(T.poff, T.ng0 + 1, (long long)i);
    const int g1 = T.partner0[g], c = (int)(T.gkey0[g] >> 32), k = T.cand_k[c];
    const int n2 = T.kpos[1][T.gstart[1][g1 + 1]] - T.kpos[1][T.gstart[1][g1]];
    const long long r = (long long)i - T.poff[g];
    const int a = (int)(r / n2), b = (int)(r % n2);
    const int l0 = (int)T.sidx[0][T.klist[0][T.kpos[0][T.gstart[0][g]] + a]] - T.ccoff[0][c];
    const int l1 = (int)T.sidx[1][T.klist[1][T.kpos[1][T.gstart[1][g1]] + b]] - T.ccoff[1][c];
    const u64 key = L.keys[k];
    const Align a1 = unpack(side_id(key, 0), L.pay[0][L.off[0][k] + l0]), a2 = unpack(side_id(key, 1), L.pay[1][L.off[1][k] + l1]);
    int s1, e1, s2, e2;
    strand_remap(a1, s1, e1);
    strand_remap(a2, s2, e2);
    pairs[i] = cmp_pair{l0, l1};
    x[i] = (double)e1;
    y[i] = (double)e2;
    u[i] = (fragment_mean - (double)(e1 - s1 + 1)) - (double)(e2 - s2 + 1);        // DoClustering :554-556: the lengths are ints
    // descending coordinate inside the problem; x and y are ints, so the key holds them whole
    const u64 p = (u64)T.pidx[c] << 32;
    xkey[i] = p | (0xFFFFFFFFu - ordered(e1));
    ykey[i] = p | (0xFFFFFFFFu - ordered(e2));
    val[i] = (uint32_t)i;
}

// after the stable sort by (problem, coordinate descending): position q holds mate pair val[q], q - prob_off is its rank
__global__ void k_ranks(const u64* __restrict__ skey, const uint32_t* __restrict__ sval, const long long* __restrict__ prob_off, int64_t n_mp,
                        int32_t* __restrict__ rank)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n_mp) rank[sval[q]] = (int32_t)(q - prob_off[skey[q] >> 32]);
}

// ---- the lines to print (:549-583)
// one lane per fragment group [g0, g1) of the problems of the range (groups are sorted by bin pair, so these are theirs and
// those of the candidates between them that did not survive): a mate pair is selected for cluster j if its bit is set and no
// earlier mate pair of the group had it
__global__ void k_select_masks(GroupTables T, int64_t g0, int64_t g1, int64_t p0, int64_t lo, int64_t hi, const int32_t* __restrict__ ncl,
                               const uint16_t* __restrict__ member, uint16_t* __restrict__ sel, int* __restrict__ cnt)
{
    const int64_t g = g0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g == g0) cnt[hi - lo] = 0;
    if (g >= g1) return;
    const long long a = T.poff[g], b = T.poff[g + 1];
    if (a == b || a < lo || b > hi) return;                         // no mate pairs; (none lies outside the range)
    const int n = ncl[T.pidx[T.gkey0[g] >> 32] - p0];
    const unsigned mask = n >= 16 ? 0xFFFFu : n <= 0 ? 0u : (1u << n) - 1u;
    unsigned seen = 0;
    for (long long i = a; i < b; ++i) {
        const unsigned m = member[i - lo] & mask;
        const unsigned take = m & ~seen;
        seen |= m;
        sel[i - lo] = (uint16_t)take;
        cnt[i - lo] = __popc(take);
    }
}

__global__ void k_select_keys(const uint16_t* __restrict__ sel, const int* __restrict__ roff, const long long* __restrict__ prob_off, int64_t p0, int64_t p1,
                              int64_t lo, int64_t hi, u64* __restrict__ key, uint32_t* __restrict__ val)
{
    const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    unsigned m = sel[i - lo];
    if (!m) return;
    // (empty problems share their offset with the next one: the owner is the last problem that starts at or before i)
    const u64 p = (u64)owner_of(prob_off + p0, p1 - p0 + 1, (long long)i);
    int at = roff[i - lo];
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        key[at] = (p << 4) | (u64)j;
        val[at] = (uint32_t)(i - lo);
        ++at;
    }
}

__global__ void k_rows(Lists L, const u64* __restrict__ skey, const uint32_t* __restrict__ sval, int64_t n_rows, int64_t p0, int64_t lo,
                       const int32_t* __restrict__ first_cluster, const int32_t* __restrict__ prob_bin, const cmp_pair* __restrict__ pairs,
                       cmp_row* __restrict__ rows)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rows) return;
    const int64_t i = lo + sval[q], p = (int64_t)(skey[q] >> 4);
    const int j = (int)(skey[q] & 15u), k = prob_bin[p0 + p];
    const cmp_pair pr = pairs[i];
    const u64 key = L.keys[k];
    cmp_row r;
    r.cluster_id = first_cluster[p] + j;
    for (int s = 0; s < 2; ++s) {
        const Align a = unpack(side_id(key, s), L.pay[s][L.off[s][k] + (s == 0 ? pr.first : pr.second)]);
        r.fragment[s] = a.fragment;
        r.read_end[s] = a.read_end;
        r.ref[s] = a.ref;
        r.strand[s] = a.strand;
        r.start[s] = a.start;
        r.end[s] = a.end;
    }
    rows[q] = r;
}

int bits_for(int64_t n)            // bits that hold every value below n
{
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < n) ++b;
    return b;
}

struct SideWork {
    DeviceBuffer<int> clen, ccoff, glen, gstart, partner, link, kept, kpos, klist;
    DeviceBuffer<u64> key, skey, gkey;
    DeviceBuffer<uint32_t> val, sidx;
    int64_t m = 0, ng = 0;
};

}  // namespace

struct cmp_problems {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[2];
    DeviceBuffer<uint8_t> tmp;
    // uploads of cmp_problems_build_lists
    DeviceBuffer<u64> up_keys;
    DeviceBuffer<int> up_off[2];
    DeviceBuffer<cmp_packed> up_pay[2];
    Lists L{};
    bool built = false;
    // work
    DeviceBuffer<int> flag, cidx, cand_k, matched, mpre, glo, surv, pidx, n_runs;
    DeviceBuffer<long long> pcnt, poff;
    SideWork side[2];
    DeviceBuffer<u64> rkey, rkey_sorted;
    DeviceBuffer<uint32_t> rval, rval_sorted;
    int64_t nc = 0;
    // results
    DeviceBuffer<long long> prob_off;
    DeviceBuffer<int32_t> prob_bin, prob_group, to_xo, to_yo;
    DeviceBuffer<double> x, y, u;
    DeviceBuffer<cmp_pair> pairs;
    DeviceBuffer<uint16_t> member;          // the caller's, through the view
    std::vector<int64_t> h_prob_off;
    std::vector<int32_t> h_prob_group;      // the first fragment group (of `first`) of every problem, one more entry = their number
    int64_t n_problems = 0, n_mate_pairs = 0;
    // select
    DeviceBuffer<int32_t> ncl, first_cluster;
    DeviceBuffer<uint16_t> sel;
    DeviceBuffer<int> cnt, roff;
    DeviceBuffer<cmp_row> rows;
    int64_t n_rows = -1;
};

namespace {

hipError_t scan_int(cmp_problems* P, const int* in, int* out, int64_t n)
{
    hipStream_t st = P->st;
    return hiphost::cub_run(P->tmp, [&](void* t, size_t& tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, in, out, (int)n, st); });
}

GroupTables tables_of(cmp_problems* P)
{
    GroupTables T{};
    T.gkey0 = P->side[0].gkey.p;
    T.partner0 = P->side[0].partner.p;
    for (int s = 0; s < 2; ++s) {
        T.gstart[s] = P->side[s].gstart.p;
        T.kpos[s] = P->side[s].kpos.p;
        T.klist[s] = P->side[s].klist.p;
        T.ccoff[s] = P->side[s].ccoff.p;
        T.sidx[s] = P->side[s].sidx.p;
    }
    T.cand_k = P->cand_k.p;
    T.pidx = P->pidx.p;
    T.poff = P->poff.p;
    T.ng0 = P->side[0].ng;
    return T;
}

// the steps of the file comment on P->L
int build_on_device(cmp_problems* P, int64_t nk, int mfr, int mcs, double fragment_mean, cmp_problem_counts* counts)
{
    hipStream_t st = P->st;
    const Lists L = P->L;
    *counts = cmp_problem_counts{};
    P->built = false;
    P->n_rows = -1;
    P->n_problems = P->n_mate_pairs = 0;
    P->nc = 0;
    P->side[0].ng = P->side[1].ng = 0;
    P->h_prob_off.assign(1, 0);
    P->h_prob_group.assign(1, 0);
    CMP_HIP(P->prob_off.reserve(1));
    CMP_HIP(hipEventRecord(P->ev[0], st));
    CMP_HIP(hipMemsetAsync(P->prob_off.p, 0, sizeof(long long), st));
    auto finish = [&]() -> int {
        CMP_HIP(hipEventRecord(P->ev[1], st));
        CMP_HIP(hipStreamSynchronize(st));
        CMP_HIP(hipGetLastError());
        counts->n_candidates = P->nc;
        counts->n_problems = P->n_problems;
        counts->n_mate_pairs = P->n_mate_pairs;
        counts->device_ms = hiphost::elapsed(P->ev[0], P->ev[1]);
        P->built = true;
        return DSA_OK;
    };
    if (nk == 0) return finish();

    // candidates
    CMP_HIP(P->flag.reserve((size_t)nk + 1));
    CMP_HIP(P->cidx.reserve((size_t)nk + 1));
    hipLaunchKernelGGL(k_candidates, dim3(grid_of(nk + 1)), dim3(256), 0, st, L, nk, mcs, P->flag.p);
    CMP_HIP(scan_int(P, P->flag.p, P->cidx.p, nk + 1));
    int nc = 0;
    CMP_HIP(hipMemcpyAsync(&nc, P->cidx.p + nk, sizeof(int), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipStreamSynchronize(st));
    P->nc = nc;
    if (nc == 0) return finish();
    CMP_HIP(P->cand_k.reserve((size_t)nc));
    for (int s = 0; s < 2; ++s) {
        CMP_HIP(P->side[s].clen.reserve((size_t)nc + 1));
        CMP_HIP(P->side[s].ccoff.reserve((size_t)nc + 1));
    }
    hipLaunchKernelGGL(k_compact_candidates, dim3(grid_of(nk)), dim3(256), 0, st, L, nk, P->flag.p, P->cidx.p, (int64_t)nc, P->cand_k.p,
                       P->side[0].clen.p, P->side[1].clen.p);
    int m[2] = {0, 0};
    for (int s = 0; s < 2; ++s) {
        CMP_HIP(scan_int(P, P->side[s].clen.p, P->side[s].ccoff.p, (int64_t)nc + 1));
        CMP_HIP(hipMemcpyAsync(&m[s], P->side[s].ccoff.p + nc, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    CMP_HIP(hipStreamSynchronize(st));

    // grouping by (candidate, fragment), list order kept inside a group
    CMP_HIP(P->n_runs.reserve(2));
    int ng[2] = {0, 0};
    const int key_bits = 32 + bits_for(nc);
    for (int s = 0; s < 2; ++s) {
        SideWork& W = P->side[s];
        W.m = m[s];
        const size_t n = (size_t)m[s];
        CMP_HIP(W.key.reserve(n)); CMP_HIP(W.skey.reserve(n)); CMP_HIP(W.val.reserve(n)); CMP_HIP(W.sidx.reserve(n));
        CMP_HIP(W.gkey.reserve(n)); CMP_HIP(W.glen.reserve(n + 1)); CMP_HIP(W.gstart.reserve(n + 1));
        CMP_HIP(W.link.reserve(n)); CMP_HIP(W.kept.reserve(n + 1)); CMP_HIP(W.kpos.reserve(n + 1)); CMP_HIP(W.klist.reserve(n));
        if (n == 0) continue;                                    // (min_cluster_size <= 0 admits empty lists)
        hipLaunchKernelGGL(k_entry_keys, dim3(grid_of((int64_t)n)), dim3(256), 0, st, L.pay[s], L.off[s], P->cand_k.p, W.ccoff.p, (int64_t)nc,
                           (int64_t)n, W.key.p, W.val.p);
        CMP_HIP(hiphost::cub_run(P->tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceRadixSort::SortPairs(t, tb, W.key.p, W.skey.p, W.val.p, W.sidx.p, (int)n, 0, key_bits, st);
        }));
        CMP_HIP(hiphost::cub_run(P->tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceRunLengthEncode::Encode(t, tb, W.skey.p, W.gkey.p, W.glen.p, P->n_runs.p + s, (int)n, st);
        }));
        CMP_HIP(hipMemcpyAsync(&ng[s], P->n_runs.p + s, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    CMP_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < 2; ++s) {
        SideWork& W = P->side[s];
        W.ng = ng[s];
        CMP_HIP(W.partner.reserve((size_t)ng[s]));
        CMP_HIP(hipMemsetAsync(W.glen.p + ng[s], 0, sizeof(int), st));
        CMP_HIP(scan_int(P, W.glen.p, W.gstart.p, (int64_t)ng[s] + 1));
    }
    // matching, the filter, the kept entries of every group as a compact list
    for (int s = 0; s < 2; ++s) {
        SideWork &W = P->side[s], &O = P->side[1 - s];
        if (W.ng) {
            hipLaunchKernelGGL(k_match, dim3(grid_of(W.ng)), dim3(256), 0, st, W.gkey.p, W.ng, O.gkey.p, O.ng, W.partner.p);
            hipLaunchKernelGGL(k_filter, dim3(grid_of(W.ng, 64)), dim3(64), 0, st, L, s, mfr, P->cand_k.p, W.ccoff.p, W.gkey.p, W.gstart.p, W.partner.p,
                               W.ng, W.sidx.p, W.link.p, W.kept.p);
        }
        CMP_HIP(hipMemsetAsync(W.kept.p + W.m, 0, sizeof(int), st));
        CMP_HIP(scan_int(P, W.kept.p, W.kpos.p, W.m + 1));
        if (W.m) hipLaunchKernelGGL(k_kept_list, dim3(grid_of(W.m)), dim3(256), 0, st, W.kept.p, W.kpos.p, W.m, W.klist.p);
    }
    // problems
    const int64_t ng0 = P->side[0].ng;
    CMP_HIP(P->matched.reserve((size_t)ng0 + 1));
    CMP_HIP(P->mpre.reserve((size_t)ng0 + 1));
    CMP_HIP(P->glo.reserve((size_t)nc));
    CMP_HIP(P->surv.reserve((size_t)nc + 1));
    CMP_HIP(P->pidx.reserve((size_t)nc + 1));
    CMP_HIP(P->pcnt.reserve((size_t)ng0 + 1));
    CMP_HIP(P->poff.reserve((size_t)ng0 + 1));
    hipLaunchKernelGGL(k_matched_flags, dim3(grid_of(ng0 + 1)), dim3(256), 0, st, P->side[0].partner.p, ng0, P->matched.p);
    CMP_HIP(scan_int(P, P->matched.p, P->mpre.p, ng0 + 1));
    hipLaunchKernelGGL(k_survivors, dim3(grid_of((int64_t)nc + 1)), dim3(256), 0, st, P->side[0].gkey.p, ng0, P->mpre.p, (int64_t)nc, mcs, P->glo.p,
                       P->surv.p);
    CMP_HIP(scan_int(P, P->surv.p, P->pidx.p, (int64_t)nc + 1));
    hipLaunchKernelGGL(k_pair_counts, dim3(grid_of(ng0 + 1)), dim3(256), 0, st, P->side[0].gkey.p, P->side[0].partner.p, ng0, P->surv.p,
                       P->side[0].gstart.p, P->side[0].kpos.p, P->side[1].gstart.p, P->side[1].kpos.p, P->pcnt.p);
    CMP_HIP(hiphost::cub_run(P->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::ExclusiveSum(t, tb, P->pcnt.p, P->poff.p, (int)(ng0 + 1), st);
    }));
    int np = 0;
    long long n_mp = 0;
    CMP_HIP(hipMemcpyAsync(&np, P->pidx.p + nc, sizeof(int), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipMemcpyAsync(&n_mp, P->poff.p + ng0, sizeof(long long), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipStreamSynchronize(st));
    CMP_HIP(P->prob_off.reserve((size_t)np + 1));
    CMP_HIP(P->prob_bin.reserve((size_t)np));
    CMP_HIP(P->prob_group.reserve((size_t)np + 1));
    hipLaunchKernelGGL(k_problem_table, dim3(grid_of(nc)), dim3(256), 0, st, P->surv.p, P->pidx.p, P->glo.p, P->cand_k.p, P->poff.p, (int64_t)nc, ng0,
                       (int64_t)np, P->prob_off.p, P->prob_bin.p, P->prob_group.p);
    P->h_prob_off.assign((size_t)np + 1, 0);
    P->h_prob_group.assign((size_t)np + 1, 0);
    CMP_HIP(hipMemcpyAsync(P->h_prob_off.data(), P->prob_off.p, ((size_t)np + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipMemcpyAsync(P->h_prob_group.data(), P->prob_group.p, ((size_t)np + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipStreamSynchronize(st));
    for (int p = 0; p < np; ++p)
        if (P->h_prob_off[(size_t)p + 1] - P->h_prob_off[(size_t)p] > INT32_MAX)
            return hiphost::fail(cmp_err(), DSA_E_LIMIT, "a bin pair with more than 2^31 - 1 mate pairs");
    if (n_mp > INT32_MAX) return hiphost::fail(cmp_err(), DSA_E_LIMIT, "more than 2^31 - 1 mate pairs in one build");
    P->n_problems = np;
    P->n_mate_pairs = n_mp;
    if (n_mp == 0) return finish();

    // mate pairs and ranks
    const size_t n = (size_t)n_mp;
    CMP_HIP(P->pairs.reserve(n)); CMP_HIP(P->x.reserve(n)); CMP_HIP(P->y.reserve(n)); CMP_HIP(P->u.reserve(n));
    CMP_HIP(P->to_xo.reserve(n)); CMP_HIP(P->to_yo.reserve(n)); CMP_HIP(P->member.reserve(n));
    // (two keys per mate pair: the x keys in rkey, the y keys behind them)
    CMP_HIP(P->rkey.reserve(2 * n)); CMP_HIP(P->rkey_sorted.reserve(n)); CMP_HIP(P->rval.reserve(n)); CMP_HIP(P->rval_sorted.reserve(n));
    hipLaunchKernelGGL(k_mate_pairs, dim3(grid_of(n_mp)), dim3(256), 0, st, L, tables_of(P), (int64_t)n_mp, fragment_mean, P->pairs.p, P->x.p, P->y.p,
                       P->u.p, P->rkey.p, P->rkey.p + n, P->rval.p);
    const int rank_bits = 32 + bits_for(np);
    for (int w = 0; w < 2; ++w) {
        CMP_HIP(hiphost::cub_run(P->tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceRadixSort::SortPairs(t, tb, P->rkey.p + (w ? n : 0), P->rkey_sorted.p, P->rval.p, P->rval_sorted.p, (int)n, 0, rank_bits, st);
        }));
        hipLaunchKernelGGL(k_ranks, dim3(grid_of(n_mp)), dim3(256), 0, st, P->rkey_sorted.p, P->rval_sorted.p, P->prob_off.p, (int64_t)n_mp,
                           w ? P->to_yo.p : P->to_xo.p);
    }
    return finish();
}

}  // namespace

extern "C" {

int cmp_problems_create(cmp_problems** out, int device)
{
    if (!out) return DSA_E_ARG;
    *out = nullptr;
    if (hiphost::check_device(device, &cmp_err())) return DSA_E_DEVICE;
    CMP_HIP(hipSetDevice(device));
    cmp_problems* p = new cmp_problems();
    p->device = device;
    if (p->st.create(hipStreamNonBlocking) != hipSuccess || p->ev[0].create() != hipSuccess || p->ev[1].create() != hipSuccess) {
        delete p;
        cmp_err() = "cannot create a stream";
        return DSA_E_DEVICE;
    }
    *out = p;
    return DSA_OK;
}

void cmp_problems_destroy(cmp_problems* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

int cmp_problems_build(cmp_problems* p, cmp_binner* b, int32_t mfr, int32_t mcs, double fragment_mean, cmp_problem_counts* counts)
{
    if (!p || !b || !counts || mfr <= 0) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build: null pointer or min_fusion_range <= 0");
    if (!b->ran) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build before a successful cmp_bin_run");
    if (b->device != p->device) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build: the binner is on device %d, the problems on %d", b->device, p->device);
    CMP_HIP(hipSetDevice(p->device));
    p->L.keys = b->side[0].uniq.p;
    for (int s = 0; s < 2; ++s) {
        p->L.off[s] = (const int*)b->side[s].off.p;
        p->L.pay[s] = b->side[s].pay_sorted.p;
    }
    return build_on_device(p, b->n_keys, mfr, mcs, fragment_mean, counts);
}

int cmp_problems_build_lists(cmp_problems* p, const uint64_t* keys, const int64_t* off_first, const int64_t* off_second, const cmp_packed* first,
                             const cmp_packed* second, int64_t n_keys, int32_t mfr, int32_t mcs, double fragment_mean, cmp_problem_counts* counts)
{
    if (!p || !counts || mfr <= 0 || n_keys < 0 || (n_keys && (!keys || !off_first || !off_second)))
        return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build_lists: null pointer, negative count or min_fusion_range <= 0");
    const int64_t* offs[2] = {off_first, off_second};
    const cmp_packed* pays[2] = {first, second};
    std::vector<int> off32[2];
    for (int s = 0; s < 2 && n_keys; ++s) {
        off32[s].resize((size_t)n_keys + 1);
        if (offs[s][0] != 0) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build_lists: offsets do not start at 0");
        for (int64_t k = 0; k <= n_keys; ++k) {
            if ((k && offs[s][k] < offs[s][k - 1]) || offs[s][k] > INT32_MAX)
                return hiphost::fail(cmp_err(), offs[s][k] > INT32_MAX ? DSA_E_LIMIT : DSA_E_ARG, "cmp_problems_build_lists: offsets descend or pass 2^31 - 1");
            off32[s][(size_t)k] = (int)offs[s][k];
        }
        if (off32[s][(size_t)n_keys] && !pays[s]) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build_lists: null list");
    }
    for (int64_t k = 1; k < n_keys; ++k)
        if (keys[k] <= keys[k - 1]) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_build_lists: keys not ascending");
    CMP_HIP(hipSetDevice(p->device));
    if (n_keys) {
        CMP_HIP(p->up_keys.reserve((size_t)n_keys));
        CMP_HIP(hipMemcpy(p->up_keys.p, keys, (size_t)n_keys * sizeof(uint64_t), hipMemcpyHostToDevice));
        for (int s = 0; s < 2; ++s) {
            const size_t n = (size_t)off32[s][(size_t)n_keys];
            CMP_HIP(p->up_off[s].reserve((size_t)n_keys + 1));
            CMP_HIP(p->up_pay[s].reserve(n));
            CMP_HIP(hipMemcpy(p->up_off[s].p, off32[s].data(), ((size_t)n_keys + 1) * sizeof(int), hipMemcpyHostToDevice));
            if (n) CMP_HIP(hipMemcpy(p->up_pay[s].p, pays[s], n * sizeof(cmp_packed), hipMemcpyHostToDevice));
            p->L.off[s] = p->up_off[s].p;
            p->L.pay[s] = p->up_pay[s].p;
        }
        p->L.keys = p->up_keys.p;
    }
    return build_on_device(p, n_keys, mfr, mcs, fragment_mean, counts);
}

int cmp_problems_fetch(cmp_problems* p, int64_t* prob_off, double* x, double* y, double* u, int32_t* to_xo, int32_t* to_yo, cmp_pair* pairs,
                       int32_t* bin_pair)
{
    if (!p || !p->built) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_fetch before a successful build");
    CMP_HIP(hipSetDevice(p->device));
    const size_t np = (size_t)p->n_problems, n = (size_t)p->n_mate_pairs;
    if (prob_off) memcpy(prob_off, p->h_prob_off.data(), (np + 1) * sizeof(int64_t));
    if (bin_pair && np) CMP_HIP(hipMemcpy(bin_pair, p->prob_bin.p, np * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (!n) return DSA_OK;
    if (x) CMP_HIP(hipMemcpy(x, p->x.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (y) CMP_HIP(hipMemcpy(y, p->y.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (u) CMP_HIP(hipMemcpy(u, p->u.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (to_xo) CMP_HIP(hipMemcpy(to_xo, p->to_xo.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (to_yo) CMP_HIP(hipMemcpy(to_yo, p->to_yo.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pairs) CMP_HIP(hipMemcpy(pairs, p->pairs.p, n * sizeof(cmp_pair), hipMemcpyDeviceToHost));
    return DSA_OK;
}

int cmp_problems_view(const cmp_problems* p, cmp_problems_device* out)
{
    if (!p || !out || !p->built) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_view before a successful build");
    *out = cmp_problems_device{};
    out->prob_off = (const int64_t*)p->prob_off.p;
    out->x = p->x.p;
    out->y = p->y.p;
    out->u = p->u.p;
    out->to_xo = p->to_xo.p;
    out->to_yo = p->to_yo.p;
    out->pairs = p->pairs.p;
    out->bin_pair = p->prob_bin.p;
    out->member = p->member.p;
    out->n_problems = p->n_problems;
    out->n_mate_pairs = p->n_mate_pairs;
    out->device = p->device;
    return DSA_OK;
}

int cmp_problems_select(cmp_problems* p, int64_t p0, int64_t p1, const int32_t* n_clusters, const uint16_t* member, int32_t cluster_base, int64_t* n_rows)
{
    if (!p || !n_rows || !p->built) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_select before a successful build");
    if (p0 < 0 || p1 < p0 || p1 > p->n_problems || (p1 > p0 && !n_clusters))
        return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_select: problems [%lld, %lld) of %lld", (long long)p0, (long long)p1, (long long)p->n_problems);
    CMP_HIP(hipSetDevice(p->device));
    hipStream_t st = p->st;
    *n_rows = 0;
    p->n_rows = 0;
    const int64_t lo = p->h_prob_off[(size_t)p0], hi = p->h_prob_off[(size_t)p1], n = hi - lo, np = p1 - p0;
    if (n == 0) return DSA_OK;
    if (!member) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_select: null member masks");
    std::vector<int32_t> first((size_t)np);
    int64_t id = cluster_base;
    for (int64_t q = 0; q < np; ++q) {
        if (n_clusters[q] < 0 || n_clusters[q] > 16) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_select: n_clusters[%lld] = %d", (long long)q, n_clusters[q]);
        first[(size_t)q] = (int32_t)id;
        id += n_clusters[q];
    }
    if (id > INT32_MAX) return hiphost::fail(cmp_err(), DSA_E_LIMIT, "cluster ids pass 2^31 - 1");
    CMP_HIP(p->ncl.reserve((size_t)np));
    CMP_HIP(p->first_cluster.reserve((size_t)np));
    CMP_HIP(p->sel.reserve((size_t)n));
    CMP_HIP(p->cnt.reserve((size_t)n + 1));
    CMP_HIP(p->roff.reserve((size_t)n + 1));
    CMP_HIP(hipMemcpyAsync(p->ncl.p, n_clusters, (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice, st));
    CMP_HIP(hipMemcpyAsync(p->first_cluster.p, first.data(), (size_t)np * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const GroupTables T = tables_of(p);
    const int64_t g0 = p->h_prob_group[(size_t)p0], g1 = p->h_prob_group[(size_t)p1];
    hipLaunchKernelGGL(k_select_masks, dim3(grid_of(std::max<int64_t>(g1 - g0, 1), 64)), dim3(64), 0, st, T, g0, g1, p0, lo, hi, p->ncl.p, member,
                       p->sel.p, p->cnt.p);
    CMP_HIP(scan_int(p, p->cnt.p, p->roff.p, n + 1));
    int rows = 0;
    CMP_HIP(hipMemcpyAsync(&rows, p->roff.p + n, sizeof(int), hipMemcpyDeviceToHost, st));
    CMP_HIP(hipStreamSynchronize(st));                      // (first[] has been read by now, too)
    CMP_HIP(hipGetLastError());
    if (rows < 0) return hiphost::fail(cmp_err(), DSA_E_LIMIT, "more than 2^31 - 1 rows in one select: give fewer problems per call");
    if (rows) {
        const size_t r = (size_t)rows;
        CMP_HIP(p->rkey.reserve(r)); CMP_HIP(p->rkey_sorted.reserve(r)); CMP_HIP(p->rval.reserve(r)); CMP_HIP(p->rval_sorted.reserve(r));
        CMP_HIP(p->rows.reserve(r));
        hipLaunchKernelGGL(k_select_keys, dim3(grid_of(n)), dim3(256), 0, st, p->sel.p, p->roff.p, p->prob_off.p, p0, p1, lo, hi, p->rkey.p, p->rval.p);
        CMP_HIP(hiphost::cub_run(p->tmp, [&](void* t, size_t& tb) {
            return hipcub::DeviceRadixSort::SortPairs(t, tb, p->rkey.p, p->rkey_sorted.p, p->rval.p, p->rval_sorted.p, rows, 0, 4 + bits_for(np + 1), st);
        }));
        hipLaunchKernelGGL(k_rows, dim3(grid_of(rows)), dim3(256), 0, st, p->L, p->rkey_sorted.p, p->rval_sorted.p, (int64_t)rows, p0, lo, p->first_cluster.p,
                           p->prob_bin.p, p->pairs.p, p->rows.p);
        CMP_HIP(hipStreamSynchronize(st));
        CMP_HIP(hipGetLastError());
    }
    p->n_rows = rows;
    *n_rows = rows;
    return DSA_OK;
}

int cmp_problems_rows(cmp_problems* p, cmp_row* rows, int64_t cap, int64_t* n_rows)
{
    if (!p || !n_rows || cap < 0) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_rows: null pointer or negative capacity");
    if (p->n_rows < 0) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_rows before a successful cmp_problems_select");
    *n_rows = p->n_rows;
    if (p->n_rows > cap) return hiphost::fail(cmp_err(), DSA_E_CAPACITY, "cmp_problems_rows: %lld rows, room for %lld", (long long)p->n_rows, (long long)cap);
    if (p->n_rows == 0) return DSA_OK;
    if (!rows) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmp_problems_rows: null buffer");
    CMP_HIP(hipSetDevice(p->device));
    CMP_HIP(hipMemcpy(rows, p->rows.p, (size_t)p->n_rows * sizeof(cmp_row), hipMemcpyDeviceToHost));
    return DSA_OK;
}

// (the "cmpt" section of the header; cmp_problems_select has waited for the rows, so any stream may read them)
int cmpt_problems_rows_view(cmp_problems* p, const cmp_row** rows_device, int64_t* n_rows)
{
    if (!p || !rows_device || !n_rows) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmpt_problems_rows_view: null pointer");
    *rows_device = nullptr;
    *n_rows = 0;
    if (p->n_rows < 0) return hiphost::fail(cmp_err(), DSA_E_ARG, "cmpt_problems_rows_view before a successful cmp_problems_select");
    *rows_device = p->n_rows ? p->rows.p : nullptr;
    *n_rows = p->n_rows;
    return DSA_OK;
}

}  // extern "C"
