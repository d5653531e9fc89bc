// sc_shared.hpp — what sc_api.hip shares with sct_api.hip: the kernels of the greedy set cover and the host function that runs
// them on clusters that are in device memory already and leaves owner[] there.  Internal: nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "hip_host.hpp"
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_sc.h"

namespace {

constexpr int SMALL_MAX = 32;   // components with more clusters than this get a whole wave

// occurrence k of the input -> (element key, owning cluster)
__global__ void k_occurrences(const int64_t* __restrict__ cluster_off, int32_t n_clusters, int32_t* __restrict__ occ_cluster)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clusters) return;
    for (int64_t k = cluster_off[c]; k < cluster_off[c + 1]; ++k) occ_cluster[k] = c;
}

// e2c_off[e] = first position of key e in the sorted keys (lower bound); e2c_off[max_element+1] = n
__global__ void k_lower_bounds(const int32_t* __restrict__ keys, int64_t n, int32_t max_element, int64_t* __restrict__ off)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > (int64_t)max_element + 1) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < e) lo = mid + 1; else hi = mid;
    }
    off[e] = lo;
}

__global__ void k_iota(int32_t* __restrict__ a, int32_t n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = i;
}

// root of c's tree.  label[x] <= x always (a hook only ever lowers a label), so the walk ends
__device__ __forceinline__ int root_of(const int32_t* label, int c)
{
    int r = c, p;
    while ((p = label[r]) != r) r = p;
    return r;
}

// hook: every fragment hangs the ROOTS of its clusters' trees under the smallest of them.  Lowering the label of the cluster
// itself would let a label advance one cluster per round along a chain of clusters; a root moves its whole tree.  In two
// rounds a tree either hangs under another or has taken in every tree it touched, so the trees of a component halve every
// two rounds and the number of rounds is logarithmic in the clusters, whatever the shape of the component.
__global__ void k_hook(const int64_t* __restrict__ e2c_off, const int32_t* __restrict__ e2c, int32_t max_element,
                       int32_t* label, int* __restrict__ changed)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > max_element) return;
    const int64_t b = e2c_off[e], en = e2c_off[e + 1];
    if (en - b < 2) return;
    int m = 0x7FFFFFFF;
    for (int64_t k = b; k < en; ++k) m = min(m, root_of(label, e2c[k]));
    for (int64_t k = b; k < en; ++k) {
        const int r = root_of(label, e2c[k]);
        if (r > m) {                            // m < r and in r's component: the forest stays a forest
            atomicMin(&label[r], m);
            *changed = 1;
        }
    }
}

// compress: every cluster jumps to its grandparent until its parent is a root.  No hook runs beside this kernel, so the
// roots stand still and a lane writes its own label only; the jumps of the others shorten its way.
__global__ void k_compress(int32_t* label, int32_t n)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    int p = label[c];
    for (;;) {
        const int g = label[p];
        if (g == p) break;
        label[c] = g;
        p = g;
    }
}

// segment heads of the (label-sorted) cluster list -> component table
__global__ void k_mark_heads(const int32_t* __restrict__ sorted_label, int32_t n, int32_t* __restrict__ head_flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head_flag[i] = (i == 0 || sorted_label[i] != sorted_label[i - 1]) ? 1 : 0;
}
__global__ void k_scatter_heads(const int32_t* __restrict__ head_flag, const int32_t* __restrict__ head_rank, int32_t n,
                                int32_t* __restrict__ comp_begin)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head_flag[i]) comp_begin[head_rank[i]] = i;
    if (i == n - 1) comp_begin[head_rank[i] + head_flag[i]] = n;   // end sentinel
}

struct Greedy {
    const int64_t* cluster_off;
    const int32_t* elements;
    const int64_t* e2c_off;
    const int32_t* e2c;
    const int32_t* comp_clusters;   // clusters sorted by (component, index)
    const int32_t* comp_begin;
    int32_t n_components;
    int32_t* size;
    int32_t* seq;
    int32_t* owner;
};

// assignment step of tools/setcover.cpp:76-106 for the chosen cluster
__device__ __forceinline__ void take_cluster(const Greedy& g, int best, int& counter)
{
    for (int64_t k = g.cluster_off[best]; k < g.cluster_off[best + 1]; ++k) {
        const int e = g.elements[k];
        if (g.owner[e] >= 0) continue;
        g.owner[e] = best;
        for (int64_t q = g.e2c_off[e]; q < g.e2c_off[e + 1]; ++q) {     // ascending cluster index, duplicates included
            const int c2 = g.e2c[q];
            g.size[c2] -= 1;
            g.seq[c2] = ++counter;
        }
    }
}

// one lane per small component
__global__ void k_greedy_small(Greedy g)
{
    const int comp = blockIdx.x * blockDim.x + threadIdx.x;
    if (comp >= g.n_components) return;
    const int b = g.comp_begin[comp], e = g.comp_begin[comp + 1];
    if (e - b > SMALL_MAX) return;
    int counter = 0;
    for (int i = b; i < e; ++i) {
        const int c = g.comp_clusters[i];
        g.size[c] = (int)(g.cluster_off[c + 1] - g.cluster_off[c]);
        g.seq[c] = ++counter;                        // initial arrival order: ascending cluster index
    }
    for (;;) {
        int best = -1, bs = -1, bq = -1;
        for (int i = b; i < e; ++i) {
            const int c = g.comp_clusters[i];
            const int s = g.size[c], q = g.seq[c];
            if (s > bs || (s == bs && q > bq)) { best = c; bs = s; bq = q; }
        }
        if (bs <= 0) break;
        take_cluster(g, best, counter);
    }
}

// one wave per large component: the arg-max over (size, arrival) is a wave reduction, the assignment
// step stays sequential (its order defines the arrival stamps)
__global__ void k_greedy_large(Greedy g, const int32_t* __restrict__ large_list, int32_t n_large)
{
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (wave >= n_large) return;
    const int comp = large_list[wave];
    const int b = g.comp_begin[comp], e = g.comp_begin[comp + 1];
    for (int i = b + lane; i < e; i += 64) {
        const int c = g.comp_clusters[i];
        g.size[c] = (int)(g.cluster_off[c + 1] - g.cluster_off[c]);
        g.seq[c] = i - b + 1;
    }
    int counter = e - b;
    __threadfence_block();
    for (;;) {
        long long key = -1;                           // (size << 32 | seq), cluster carried alongside
        int best = -1;
        for (int i = b + lane; i < e; i += 64) {
            const int c = g.comp_clusters[i];
            const long long k = ((long long)g.size[c] << 32) | (unsigned)g.seq[c];
            if (k > key) { key = k; best = c; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long ok = __shfl_xor(key, d, 64);
            const int ob = __shfl_xor(best, d, 64);
            if (ok > key) { key = ok; best = ob; }
        }
        if ((key >> 32) <= 0) break;                  // wave-uniform after the butterfly
        if (lane == 0) take_cluster(g, best, counter);
        __threadfence_block();
        counter = __shfl(counter, 0, 64);
    }
}

__global__ void k_collect_large(const int32_t* __restrict__ comp_begin, int32_t n_components, int32_t* __restrict__ list,
                                int32_t* __restrict__ n_large)
{
    const int comp = blockIdx.x * blockDim.x + threadIdx.x;
    if (comp >= n_components) return;
    if (comp_begin[comp + 1] - comp_begin[comp] > SMALL_MAX) list[atomicAdd(n_large, 1)] = comp;
}

// The set cover of clusters in CSR form in device memory (cluster_off: n_clusters + 1 offsets, elements: n_occ fragments, each
// in [0, max_element]; n_clusters > 0, 0 < n_occ < 2^31): owner[0 .. max_element] on the device receives every fragment's
// cluster, or -1.  Everything runs on `st`; the host waits only for the counts it steers by (a round's `changed` flag, the
// numbers of components and of large ones).  On return the stream has been synchronised and `t` holds the stages.
inline int sc_cover_device(std::string& err, hipStream_t st, const int64_t* d_coff, const int32_t* d_el, int32_t n_clusters, int64_t n_occ,
                           int32_t max_element, int32_t* d_owner, sc_timing& t)
{
#define SC_DEV_HIP(call) HIPHOST_TRY(err, call)
    using hiphost::DeviceBuffer;
    hiphost::Event ev[4];                 // destroyed on every return
    for (auto& e : ev) SC_DEV_HIP(e.create());
    DeviceBuffer<int64_t> d_e2c_off;
    DeviceBuffer<int32_t> d_occ_cluster, d_keys_sorted, d_e2c, d_label, d_label_sorted, d_idx, d_comp_clusters, d_flag, d_rank,
        d_comp_begin, d_size, d_seq, d_large, d_nlarge;
    DeviceBuffer<int> d_changed;
    DeviceBuffer<uint8_t> d_tmp;
    const int nel = max_element + 1;
    SC_DEV_HIP(d_occ_cluster.reserve(n_occ));
    SC_DEV_HIP(d_keys_sorted.reserve(n_occ)); SC_DEV_HIP(d_e2c.reserve(n_occ)); SC_DEV_HIP(d_e2c_off.reserve(nel + 2));
    SC_DEV_HIP(d_label.reserve(n_clusters)); SC_DEV_HIP(d_label_sorted.reserve(n_clusters)); SC_DEV_HIP(d_idx.reserve(n_clusters));
    SC_DEV_HIP(d_comp_clusters.reserve(n_clusters)); SC_DEV_HIP(d_flag.reserve(n_clusters)); SC_DEV_HIP(d_rank.reserve(n_clusters));
    SC_DEV_HIP(d_comp_begin.reserve(n_clusters + 2)); SC_DEV_HIP(d_size.reserve(n_clusters)); SC_DEV_HIP(d_seq.reserve(n_clusters));
    SC_DEV_HIP(d_large.reserve(n_clusters)); SC_DEV_HIP(d_nlarge.reserve(1)); SC_DEV_HIP(d_changed.reserve(1));
    SC_DEV_HIP(hipMemsetAsync(d_owner, 0xFF, nel * sizeof(int32_t), st));
    const int B = 256;
    auto grid = [&](int64_t n) { return dim3(hiphost::grid_of(n, B)); };
    auto fetch = [&](int* host, const int* dev) -> hipError_t {          // one small count to the host
        const hipError_t e = hipMemcpyAsync(host, dev, sizeof(int), hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    };

    // 1. fragment -> clusters index: stable radix sort of the occurrences by fragment keeps each list in
    //    ascending cluster order (the order tools/setcover.cpp:47-60 builds it in)
    SC_DEV_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_occurrences, grid(n_clusters), dim3(B), 0, st, d_coff, n_clusters, d_occ_cluster.p);
    size_t tmp_bytes = 0, need = 0;
    int bits = 1;
    while ((1ll << bits) <= max_element) ++bits;
    SC_DEV_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_el, d_keys_sorted.p, d_occ_cluster.p, d_e2c.p, (int)n_occ, 0, bits, st));
    tmp_bytes = need;
    int cbits = 1;
    while ((1ll << cbits) < n_clusters) ++cbits;
    SC_DEV_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need, d_label.p, d_label_sorted.p, d_idx.p, d_comp_clusters.p, n_clusters, 0, cbits, st));
    tmp_bytes = std::max(tmp_bytes, need);
    SC_DEV_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, d_flag.p, d_rank.p, n_clusters, st));
    tmp_bytes = std::max(tmp_bytes, need);
    SC_DEV_HIP(d_tmp.reserve(tmp_bytes));
    need = tmp_bytes;
    SC_DEV_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, need, d_el, d_keys_sorted.p, d_occ_cluster.p, d_e2c.p, (int)n_occ, 0, bits, st));
    hipLaunchKernelGGL(k_lower_bounds, grid(nel + 1), dim3(B), 0, st, d_keys_sorted.p, n_occ, max_element, d_e2c_off.p);
    SC_DEV_HIP(hipEventRecord(ev[1], st));

    // 2. connected components of the cluster/fragment graph: root hooking + full compression until a round hooks nothing
    hipLaunchKernelGGL(k_iota, grid(n_clusters), dim3(B), 0, st, d_label.p, n_clusters);
    int iterations = 0;
    for (;;) {
        int changed = 0;
        SC_DEV_HIP(hipMemsetAsync(d_changed.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_hook, grid(nel), dim3(B), 0, st, d_e2c_off.p, d_e2c.p, max_element, d_label.p, d_changed.p);
        hipLaunchKernelGGL(k_compress, grid(n_clusters), dim3(B), 0, st, d_label.p, n_clusters);
        SC_DEV_HIP(fetch(&changed, d_changed.p));
        ++iterations;
        if (!changed) break;
        if (iterations > 10000) { err = "connected components did not converge"; return DSA_E_DEVICE; }
    }
    // clusters grouped by component, ascending index inside a component (stable sort by label)
    hipLaunchKernelGGL(k_iota, grid(n_clusters), dim3(B), 0, st, d_idx.p, n_clusters);
    need = tmp_bytes;
    SC_DEV_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, need, d_label.p, d_label_sorted.p, d_idx.p, d_comp_clusters.p, n_clusters, 0, cbits, st));
    hipLaunchKernelGGL(k_mark_heads, grid(n_clusters), dim3(B), 0, st, d_label_sorted.p, n_clusters, d_flag.p);
    need = tmp_bytes;
    SC_DEV_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, need, d_flag.p, d_rank.p, n_clusters, st));
    hipLaunchKernelGGL(k_scatter_heads, grid(n_clusters), dim3(B), 0, st, d_flag.p, d_rank.p, n_clusters, d_comp_begin.p);
    int last_rank = 0, last_flag = 0;
    SC_DEV_HIP(fetch(&last_rank, d_rank.p + (n_clusters - 1)));
    SC_DEV_HIP(fetch(&last_flag, d_flag.p + (n_clusters - 1)));
    const int n_components = last_rank + last_flag;
    SC_DEV_HIP(hipEventRecord(ev[2], st));

    // 3. greedy, independently per component
    Greedy g{d_coff, d_el, d_e2c_off.p, d_e2c.p, d_comp_clusters.p, d_comp_begin.p, n_components, d_size.p, d_seq.p, d_owner};
    SC_DEV_HIP(hipMemsetAsync(d_nlarge.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_collect_large, grid(n_components), dim3(B), 0, st, d_comp_begin.p, n_components, d_large.p, d_nlarge.p);
    hipLaunchKernelGGL(k_greedy_small, grid(n_components), dim3(B), 0, st, g);
    int n_large = 0;
    SC_DEV_HIP(fetch(&n_large, d_nlarge.p));
    if (n_large > 0)
        hipLaunchKernelGGL(k_greedy_large, grid((int64_t)n_large * 64), dim3(B), 0, st, g, d_large.p, n_large);
    SC_DEV_HIP(hipEventRecord(ev[3], st));
    SC_DEV_HIP(hipStreamSynchronize(st));
    SC_DEV_HIP(hipGetLastError());
    t.build_ms = hiphost::elapsed(ev[0], ev[1]);
    t.components_ms = hiphost::elapsed(ev[1], ev[2]);
    t.greedy_ms = hiphost::elapsed(ev[2], ev[3]);
    t.total_ms = hiphost::elapsed(ev[0], ev[3]);
    t.n_components = n_components;
    t.n_large = n_large;
    t.cc_iterations = iterations;
    return DSA_OK;
#undef SC_DEV_HIP
}

}  // namespace
