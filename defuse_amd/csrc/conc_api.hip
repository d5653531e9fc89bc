// conc_api.hip — the concordant-cluster filter on cluster text in device memory, for gfx950 (include/defuse_task.h, section "concordant clusters"):
// prep_local_alignment_seqs.pl, localalign and `filter_column.pl VALUES 0 1` between sct_cover and taskc_dedup.
//
// Targets: taskc_regions(TASKC_INPUT) groups the lines by (id, end); taskc_api.hip hands the groups and the parsed lines over where
//   they lie.  One lane per group runs the rules of conc_shared.hpp twice: k_targets<false> counts its targets, a 64-bit exclusive sum places
//   them, k_targets<true> writes the descriptors with the key (group, rank); a radix sort by that key and k_permute give the canonical order.
// Scores: k_pairs turns the descriptors into la_api.hip's pairs (offsets into the reference's bytes, lengths, two flags); the host
//   reads them for the wave planner and la_align_pairs_device runs k_pack_pairs and k_la16 / k_la32 into the scores buffer here.
// Texts: k_decide applies the threshold with one IEEE division and measures each line and marks the clusters that print, a
//   64-bit exclusive sum and k_print give the local.align text; k_line_keep looks every input line's id up among the groups, a
//   second sum and k_gather_lines (bat_shared.hpp's span copy, 16 lanes per line) give the filtered text.
// Every per-group array is indexed below the number of groups, every per-target array below the number of targets the scan
// counted, every per-line array below the number of lines; every store into a text lies inside the bytes its scan counted.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_la.h"
#include "bat_shared.hpp"
#include "conc_shared.hpp"
#include "hip_host.hpp"
#include "la_pairs.hpp"
#include "la_score.hpp"
#include "ptext_shared.hpp"
#include "taskc_shared.hpp"

// task_api.hip, taskc_api.hip
__attribute__((visibility("hidden"))) void task_reference_device(const task_reference* r, int* device, const uint8_t** bytes, int64_t* bytes_len,
                                                                 const task_seq** seqs, int64_t* n_seqs);
__attribute__((visibility("hidden"))) int taskc_lines_device(taskc_ctx* c, bool from_dedup, taskc_lines_view* out);
__attribute__((visibility("hidden"))) int taskc_groups_device(taskc_ctx* c, taskc_groups_view* out);
__attribute__((visibility("hidden"))) int taskc_add_device(taskc_ctx* c, int device, const uint8_t* text, int64_t len);

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using u64 = unsigned long long;

thread_local std::string g_conc_err;

#define CONC_HIP(call) HIPHOST_TRY(g_conc_err, call)
#define CONC_FAIL(code, ...) hiphost::fail(g_conc_err, code, __VA_ARGS__)

constexpr int BLOCK = 256;
constexpr int LINE_GROUP = 16;                // lanes per copied line
constexpr uint32_t SIGN = 0x80000000u;
constexpr u64 NO_STOP = ~0ull;
static_assert(sizeof(conc_target) == 48 && sizeof(la_pair) == 32 && sizeof(conc_result) == 96 && sizeof(conc_timing) == 56, "layout");

// what the host reads between the stages (in: stop NO_STOP, the rest 0)
struct Summary {
    u64 stop;                   // (group << 8) | CONC_* of the lowest group that stops
    u64 n_targets;
    uint32_t limit, n_kept, n_hit, n_kept_lines, n_noncanonical, pad_;
    int64_t align_bytes, out_bytes;
};

__device__ inline int32_t key_id(u64 key) { return (int32_t)((uint32_t)(key >> 32) ^ SIGN); }
__device__ inline int32_t key_end(u64 key) { return (int32_t)((uint32_t)key ^ SIGN); }

// the end that group g is: false with `kind` set where it stops the call
__device__ inline bool group_end(const taskc_groups_view& G, const taskc_lines_view& L, int64_t g, conc_end& E, int32_t& kind, uint32_t& limit)
{
    const int64_t i = G.glast[g];
    if (i >= L.n_input_lines) {
        kind = CONC_NOT_TWO_ENDS;
        return false;
    }
    const taskc_line r = L.rec[i];
    const uint8_t* line = L.text + L.lstart[i];
    E.name = line + r.name_off;
    E.name_len = r.name_len;
    E.start = G.gmin[g];
    E.end = G.gmax[g];
    if (E.start < -TASK_MAX_COORD || E.start > TASK_MAX_COORD || E.end < -TASK_MAX_COORD || E.end > TASK_MAX_COORD) limit = 1;
    const uint8_t s = r.strand_len == 1 ? line[r.strand_off] : 0;
    if (s != '+' && s != '-') {
        kind = CONC_BAD_STRAND;
        return false;
    }
    E.strand = s == '+' ? 0 : 1;
    return true;
}

// groups 2k and 2k + 1 are ends 0 and 1 of one id
__device__ inline bool group_pair_ok(const taskc_groups_view& G, int64_t g)
{
    const int64_t a = g & ~(int64_t)1;
    return a + 1 < G.n_groups && key_id(G.key[a]) == key_id(G.key[a + 1]) && key_end(G.key[a]) == 0 && key_end(G.key[a + 1]) == 1;
}

// EMIT false: cnt[g] = the targets of group g.  EMIT true: its descriptors at off[g] .., with their keys.
template <bool EMIT>
__global__ __launch_bounds__(BLOCK) void k_targets(conc_view V, taskc_groups_view G, taskc_lines_view L, int64_t range, u64* __restrict__ cnt,
                                                    const u64* __restrict__ off, int64_t n_targets, conc_target* __restrict__ out, u64* __restrict__ key,
                                                    uint32_t* __restrict__ idx, Summary* __restrict__ sum)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= G.n_groups) return;
    int32_t kind = 0;
    uint32_t limit = 0;
    int64_t n = 0;
    conc_end me{}, other{};
    if (!group_pair_ok(G, g)) kind = CONC_NOT_TWO_ENDS;
    else if (group_end(G, L, g, me, kind, limit) && group_end(G, L, g ^ 1, other, kind, limit) && !limit) {
        const conc_end_plan P = conc_plan_end(V, me, other);
        kind = P.stop;
        int32_t lim = P.limit;
        if (!kind && !lim) {
            int64_t at = EMIT ? (int64_t)off[g] : 0;
            n = conc_end_targets(V, P, me, key_id(G.key[g]), key_end(G.key[g]), range, lim, [&](const conc_target& T, int64_t rank) {
                if (EMIT) {
                    if (at >= 0 && at < n_targets) {
                        out[at] = T;
                        key[at] = ((u64)g << 32) | (u64)rank;
                        idx[at] = (uint32_t)at;
                    }
                    ++at;
                }
            });
        }
        limit |= (uint32_t)lim;
    }
    if (!EMIT) {
        cnt[g] = (u64)n;
        if (kind) atomicMin(&sum->stop, ((u64)g << 8) | (u64)kind);          // (rare)
        if (limit) atomicOr(&sum->limit, 1u);
    }
}

__global__ void k_total(const u64* __restrict__ cnt, const u64* __restrict__ off, int64_t n, u64* __restrict__ total)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = off[n - 1] + cnt[n - 1];
}

__global__ __launch_bounds__(BLOCK) void k_permute(const conc_target* __restrict__ in, const uint32_t* __restrict__ idx, int64_t n, conc_target* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = idx[i];
    if (k < n) out[i] = in[k];
}

__global__ __launch_bounds__(BLOCK) void k_pairs(const conc_target* __restrict__ tg, int64_t n, const task_seq* __restrict__ seqs, int64_t n_seqs,
                                                  la_pair* __restrict__ pairs)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const conc_target T = tg[i];
    la_pair p{};
    if (T.seq >= 0 && T.seq < n_seqs && T.other_seq >= 0 && T.other_seq < n_seqs) {
        p.ref_off = seqs[T.seq].off + T.start;
        p.ref_len = T.len;
        p.ref_rc = T.revcomp;
        p.seq_off = seqs[T.other_seq].off + T.other_start;
        p.seq_len = T.other_len;
        p.seq_rc = T.other_rev;
    }
    pairs[i] = p;
}

// the sum of `flag` over the block onto *counter
__device__ inline void block_count(uint32_t flag, uint32_t* counter)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const uint32_t n = Reduce(tmp).Sum(flag);
    if (threadIdx.x == 0 && n) atomicAdd(counter, n);
}

// the pair (cluster) whose id is `id`, -1 if none: groups 2k are ascending by id
__device__ inline int64_t find_cluster(const taskc_groups_view& G, int32_t id)
{
    int64_t lo = 0, hi = G.n_groups / 2;
    const uint32_t want = (uint32_t)id ^ SIGN;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const uint32_t have = (uint32_t)(G.key[2 * mid] >> 32);
        if (have == want) return mid;
        if (have < want) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// localalign.cpp:84-92 for target i: printed unless (double) score / (double) max < threshold; the bytes of its line
__global__ __launch_bounds__(BLOCK) void k_decide(const conc_target* __restrict__ tg, const int32_t* __restrict__ scores, int64_t n, int32_t match,
                                                   double threshold, taskc_groups_view G, u64* __restrict__ alen, uint32_t* __restrict__ hit,
                                                   Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t keep = 0;
    if (i < n) {
        const conc_target T = tg[i];
        const int32_t score = scores[i];
        const int32_t top = (int32_t)((uint32_t)T.other_len * (uint32_t)match);
        const double percent = (double)score / (double)top;
        keep = !(percent < threshold) ? 1u : 0u;
        u64 bytes = 0;
        if (keep) {
            bytes = (u64)(taskc_dec_len(T.cluster_id) + 1 + taskc_dec_len(score) + 1 + ptext_g_length(ptext_g_of(percent)) + 1);
            const int64_t c = find_cluster(G, T.cluster_id);
            if (c >= 0) hit[c] = 1u;                                         // (every writer stores the same value)
        }
        alen[i] = bytes;
    }
    block_count(keep, &sum->n_kept);
}

__global__ __launch_bounds__(BLOCK) void k_print(const conc_target* __restrict__ tg, const int32_t* __restrict__ scores, int64_t n, int32_t match,
                                                  const u64* __restrict__ alen, const u64* __restrict__ adst, uint8_t* __restrict__ out, int64_t out_len)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || alen[i] == 0) return;
    const int64_t d = (int64_t)adst[i];
    if (d < 0 || d + (int64_t)alen[i] > out_len) return;
    const conc_target T = tg[i];
    const int32_t score = scores[i];
    const double percent = (double)score / (double)(int32_t)((uint32_t)T.other_len * (uint32_t)match);
    uint8_t* p = out + d;
    p += taskc_dec_put(T.cluster_id, p);
    *p++ = '\t';
    p += taskc_dec_put(score, p);
    *p++ = '\t';
    p += ptext_g_write(ptext_g_of(percent), p);
    *p = '\n';
}

// filter_column.pl VALUES 0 1 for input line i: kept unless its id is one that printed; its bytes with the newline
__global__ __launch_bounds__(BLOCK) void k_line_keep(taskc_lines_view L, taskc_groups_view G, const uint32_t* __restrict__ hit, u64* __restrict__ olen,
                                                      Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t keep = 0, odd = 0;
    if (i < L.n_input_lines) {
        const int32_t id = L.rec[i].id;
        const int64_t c = find_cluster(G, id);
        keep = (c >= 0 && hit[c]) ? 0u : 1u;
        olen[i] = keep ? (u64)L.llen[i] + 1u : 0u;
        // the id's text against its plain decimal (the line has a tab behind field 0: taskc_regions read eight fields)
        uint8_t dec[12];
        const int nd = taskc_dec_put(id, dec);
        const uint8_t* line = L.text + L.lstart[i];
        odd = (L.llen[i] <= nd || line[nd] != '\t') ? 1u : 0u;
        for (int k = 0; k < nd && !odd; ++k) odd = line[k] != dec[k] ? 1u : 0u;
    }
    block_count(keep, &sum->n_kept_lines);
    __syncthreads();
    block_count(odd, &sum->n_noncanonical);
}

__global__ __launch_bounds__(BLOCK) void k_count_hits(const uint32_t* __restrict__ hit, int64_t n, Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    block_count(i < n ? hit[i] : 0u, &sum->n_hit);
}

__global__ void k_text_totals(const u64* __restrict__ alen, const u64* __restrict__ adst, int64_t n, const u64* __restrict__ olen, const u64* __restrict__ odst,
                              int64_t m, Summary* __restrict__ sum)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sum->align_bytes = n ? (int64_t)(adst[n - 1] + alen[n - 1]) : 0;
        sum->out_bytes = m ? (int64_t)(odst[m - 1] + olen[m - 1]) : 0;
    }
}

// taskc_api.hip's k_gather over the lines that stay: G lanes copy one line by copy_span, the first lane without a head or tail byte
// stores the newline
template <int G>
__global__ __launch_bounds__(BLOCK) void k_gather_lines(taskc_lines_view L, const u64* __restrict__ olen, const u64* __restrict__ odst, uint8_t* __restrict__ dst,
                                                         int64_t dst_len)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t i = t / G;
    const int lane = (int)(t % G);
    if (i >= L.n_input_lines || olen[i] == 0) return;
    const int64_t src = L.lstart[i], len = L.llen[i];
    const int64_t d0 = (int64_t)odst[i], d1 = d0 + len;
    if (d0 < 0 || d1 + 1 > dst_len || src < 0 || len < 0) return;
    const int64_t n_edge = copy_span<G>(L.text, src, dst, d0, len, lane);
    if (G - 1 - lane == n_edge) dst[d1] = '\n';
}

template <class T>
int upload(DeviceBuffer<T>& buf, const T* host, int64_t n)
{
    CONC_HIP(buf.reserve((size_t)n));
    if (n) CONC_HIP(hipMemcpy(buf.p, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice));
    return DSA_OK;
}

}  // namespace

struct conc_models {
    int device = -1;
    int64_t n_seqs = 0;
    DeviceBuffer<conc_gene> genes;
    DeviceBuffer<int32_t> gene_tx, chrom_gene_first, chrom_genes, chrom_premax, seq_sorted, chrom_seq, tx_seq;
    DeviceBuffer<conc_transcript> tx;
    DeviceBuffer<conc_interval> exons, expr;
    DeviceBuffer<uint8_t> names;
    DeviceBuffer<conc_name> chrom_names, tx_names, seq_names;
    conc_view view{};           // device pointers; seqs is the reference's, set per call
};

struct conc_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[8];       // 0-2 targets, sort; 3, 4 the pairs down; 5-7 print, filter
    conc_timing timing{};
    DeviceBuffer<Summary> sum;
    Summary h_sum{};
    DeviceBuffer<uint8_t, GrowSize> tmp;
    // what conc_targets read, in place
    taskc_lines_view lines{};
    taskc_groups_view groups{};
    int64_t n_clusters = 0;
    // targets
    DeviceBuffer<u64, GrowSize> cnt, off, key[2];
    DeviceBuffer<uint32_t, GrowSize> idx[2];
    DeviceBuffer<conc_target, GrowSize> raw, tg;
    int64_t n_targets = 0;
    bool has_targets = false;
    // scores
    DeviceBuffer<la_pair, GrowSize> pairs;
    DeviceBuffer<int32_t, GrowSize> scores;
    int32_t match = 0;
    double threshold = 0.0;
    bool has_scores = false;
    // texts
    DeviceBuffer<u64, GrowSize> alen, adst, olen, odst;
    DeviceBuffer<uint32_t, GrowSize> hit;
    DeviceBuffer<uint8_t, GrowSize> atext, out;
    int64_t align_bytes = 0, out_bytes = 0;
    bool has_texts = false;
};

namespace {

int reset_summary(conc_ctx* c)
{
    CONC_HIP(c->sum.reserve(1));
    c->h_sum = Summary{};
    c->h_sum.stop = NO_STOP;
    CONC_HIP(hipMemcpyAsync(c->sum.p, &c->h_sum, sizeof(Summary), hipMemcpyHostToDevice, c->st));
    return DSA_OK;
}

int read_summary(conc_ctx* c)
{
    CONC_HIP(hipMemcpyAsync(&c->h_sum, c->sum.p, sizeof(Summary), hipMemcpyDeviceToHost, c->st));
    CONC_HIP(hipStreamSynchronize(c->st));
    CONC_HIP(hipGetLastError());
    return DSA_OK;
}

void clear_result(conc_result* r)
{
    *r = conc_result{};
    r->stop_field = -1;
}

bool name_less(const uint8_t* names, const conc_name& a, const conc_name& b) { return conc_name_cmp(names + a.off, a.len, names + b.off, b.len) < 0; }

// The argument checks of conc_models_create; nothing here touches a device.
int check_models(const conc_models_desc& d, std::vector<int32_t>& sorted)
{
    const int64_t counts[] = {d.n_genes, d.n_gene_tx, d.n_transcripts, d.n_exons, d.n_expressed, d.n_chrom_genes, d.names_len, d.n_chroms, d.n_seqs};
    for (const int64_t n : counts)
        if (n < 0 || n >= INT32_MAX) return CONC_FAIL(DSA_E_ARG, "conc_models_create: a count of %lld", (long long)n);
    if ((d.n_genes && !d.genes) || (d.n_gene_tx && !d.gene_tx) || (d.n_transcripts && (!d.transcripts || !d.transcript_names)) || (d.n_exons && !d.exons) ||
        (d.n_expressed && !d.expressed) || !d.chrom_gene_first || (d.n_chrom_genes && !d.chrom_genes) || (d.names_len && !d.names) ||
        (d.n_chroms && !d.chrom_names) || (d.n_seqs && !d.seq_names))
        return CONC_FAIL(DSA_E_ARG, "conc_models_create: null pointer with non-zero size");
    auto check_names = [&](const conc_name* t, int64_t n, const char* what, bool ascending) -> int {
        for (int64_t k = 0; k < n; ++k) {
            if (t[k].off < 0 || t[k].len < 0 || t[k].off + t[k].len > d.names_len) return CONC_FAIL(DSA_E_ARG, "conc_models_create: %s name %lld lies outside the names", what, (long long)k);
            if (conc_name_is_range(d.names + t[k].off, t[k].len)) return CONC_FAIL(DSA_E_LIMIT, "conc_models_create: %s name %lld has the form name:a-b", what, (long long)k);
            if (ascending && k > 0 && !name_less(d.names, t[k - 1], t[k])) return CONC_FAIL(DSA_E_ARG, "conc_models_create: %s names do not ascend at %lld", what, (long long)k);
        }
        return DSA_OK;
    };
    if (const int rc = check_names(d.chrom_names, d.n_chroms, "chromosome", true)) return rc;
    if (const int rc = check_names(d.transcript_names, d.n_transcripts, "transcript", true)) return rc;
    if (const int rc = check_names(d.seq_names, d.n_seqs, "sequence", false)) return rc;
    sorted.assign((size_t)d.n_seqs, 0);                 // (the FASTA index keeps one of two sequences with one name: such input is refused)
    for (int64_t k = 0; k < d.n_seqs; ++k) sorted[(size_t)k] = (int32_t)k;
    std::stable_sort(sorted.begin(), sorted.end(), [&](int32_t a, int32_t b) { return name_less(d.names, d.seq_names[a], d.seq_names[b]); });
    for (size_t k = 1; k < sorted.size(); ++k)
        if (!name_less(d.names, d.seq_names[sorted[k - 1]], d.seq_names[sorted[k]])) return CONC_FAIL(DSA_E_ARG, "conc_models_create: two sequences have one name");
    auto coord_ok = [](int32_t v) { return v >= -TASK_MAX_COORD && v <= TASK_MAX_COORD; };
    for (int64_t g = 0; g < d.n_genes; ++g) {
        const conc_gene& G = d.genes[g];
        if (G.tx_first < 0 || G.tx_count < 0 || (int64_t)G.tx_first + G.tx_count > d.n_gene_tx) return CONC_FAIL(DSA_E_ARG, "conc_models_create: gene %lld: transcripts outside gene_tx", (long long)g);
        if (!coord_ok(G.start) || !coord_ok(G.end)) return CONC_FAIL(DSA_E_LIMIT, "conc_models_create: gene %lld: a coordinate beyond TASK_MAX_COORD", (long long)g);
    }
    for (int64_t k = 0; k < d.n_gene_tx; ++k)
        if (d.gene_tx[k] < 0 || d.gene_tx[k] >= d.n_transcripts) return CONC_FAIL(DSA_E_ARG, "conc_models_create: gene_tx[%lld] is no transcript", (long long)k);
    for (int64_t t = 0; t < d.n_transcripts; ++t) {
        const conc_transcript& T = d.transcripts[t];
        if (T.gene < 0 || T.gene >= d.n_genes || T.chrom < 0 || T.chrom >= d.n_chroms || T.strand < 0 || T.strand > 2)
            return CONC_FAIL(DSA_E_ARG, "conc_models_create: transcript %lld: gene, chromosome or strand outside its table", (long long)t);
        if (T.exon_first < 0 || T.exon_count < 1 || (int64_t)T.exon_first + T.exon_count > d.n_exons || T.expr_first < 0 || T.expr_count < 0 ||
            (int64_t)T.expr_first + T.expr_count > d.n_expressed)
            return CONC_FAIL(DSA_E_ARG, "conc_models_create: transcript %lld: no exon, or intervals outside their table", (long long)t);
        int64_t length = 0;
        for (int32_t k = 0; k < T.exon_count; ++k) {
            const conc_interval& e = d.exons[T.exon_first + k];
            if (k > 0 && e.start < d.exons[T.exon_first + k - 1].start) return CONC_FAIL(DSA_E_ARG, "conc_models_create: transcript %lld: exons not sorted by start", (long long)t);
            length += std::llabs((long long)e.end - e.start + 1);
        }
        if (length > TASK_MAX_COORD) return CONC_FAIL(DSA_E_LIMIT, "conc_models_create: transcript %lld: exons longer than TASK_MAX_COORD", (long long)t);
    }
    for (const conc_interval* tab : {d.exons, d.expressed})
        for (int64_t k = 0, n = tab == d.exons ? d.n_exons : d.n_expressed; k < n; ++k)
            if (!coord_ok(tab[k].start) || !coord_ok(tab[k].end)) return CONC_FAIL(DSA_E_LIMIT, "conc_models_create: an interval beyond TASK_MAX_COORD");
    if (d.chrom_gene_first[0] != 0 || d.chrom_gene_first[d.n_chroms] != d.n_chrom_genes) return CONC_FAIL(DSA_E_ARG, "conc_models_create: chrom_gene_first does not span chrom_genes");
    for (int64_t c = 0; c < d.n_chroms; ++c) {
        if (d.chrom_gene_first[c] > d.chrom_gene_first[c + 1]) return CONC_FAIL(DSA_E_ARG, "conc_models_create: chrom_gene_first descends at %lld", (long long)c);
        for (int64_t k = d.chrom_gene_first[c]; k < d.chrom_gene_first[c + 1]; ++k) {
            if (d.chrom_genes[k] < 0 || d.chrom_genes[k] >= d.n_genes) return CONC_FAIL(DSA_E_ARG, "conc_models_create: chrom_genes[%lld] is no gene", (long long)k);
            if (k > d.chrom_gene_first[c] && d.genes[d.chrom_genes[k]].start < d.genes[d.chrom_genes[k - 1]].start)
                return CONC_FAIL(DSA_E_ARG, "conc_models_create: the genes of chromosome %lld do not ascend by start", (long long)c);
        }
    }
    return DSA_OK;
}

int build_models(conc_models* m, const conc_models_desc& d, const std::vector<int32_t>& sorted)
{
    // host tables beside `sorted`, the sequences by name (check_models): the sequence of every chromosome and transcript, the running
    // maximum of the gene ends
    std::vector<int32_t> chrom_seq((size_t)d.n_chroms, -1), tx_seq((size_t)d.n_transcripts, -1), premax((size_t)d.n_chrom_genes);
    for (int64_t c = 0; c < d.n_chroms; ++c)
        chrom_seq[(size_t)c] = conc_find_name(d.names, d.seq_names, sorted.data(), (int32_t)d.n_seqs, d.names + d.chrom_names[c].off, d.chrom_names[c].len);
    for (int64_t t = 0; t < d.n_transcripts; ++t)
        tx_seq[(size_t)t] = conc_find_name(d.names, d.seq_names, sorted.data(), (int32_t)d.n_seqs, d.names + d.transcript_names[t].off, d.transcript_names[t].len);
    for (int64_t c = 0; c < d.n_chroms; ++c)
        for (int64_t k = d.chrom_gene_first[c]; k < d.chrom_gene_first[c + 1]; ++k) {
            const int32_t end = d.genes[d.chrom_genes[k]].end;
            premax[(size_t)k] = k > d.chrom_gene_first[c] ? std::max(premax[(size_t)k - 1], end) : end;
        }
    if (const int rc = upload(m->genes, d.genes, d.n_genes)) return rc;
    if (const int rc = upload(m->gene_tx, d.gene_tx, d.n_gene_tx)) return rc;
    if (const int rc = upload(m->tx, d.transcripts, d.n_transcripts)) return rc;
    if (const int rc = upload(m->exons, d.exons, d.n_exons)) return rc;
    if (const int rc = upload(m->expr, d.expressed, d.n_expressed)) return rc;
    if (const int rc = upload(m->chrom_gene_first, d.chrom_gene_first, d.n_chroms + 1)) return rc;
    if (const int rc = upload(m->chrom_genes, d.chrom_genes, d.n_chrom_genes)) return rc;
    if (const int rc = upload(m->chrom_premax, premax.data(), d.n_chrom_genes)) return rc;
    if (const int rc = upload(m->names, d.names, d.names_len)) return rc;
    if (const int rc = upload(m->chrom_names, d.chrom_names, d.n_chroms)) return rc;
    if (const int rc = upload(m->tx_names, d.transcript_names, d.n_transcripts)) return rc;
    if (const int rc = upload(m->seq_names, d.seq_names, d.n_seqs)) return rc;
    if (const int rc = upload(m->seq_sorted, sorted.data(), d.n_seqs)) return rc;
    if (const int rc = upload(m->chrom_seq, chrom_seq.data(), d.n_chroms)) return rc;
    if (const int rc = upload(m->tx_seq, tx_seq.data(), d.n_transcripts)) return rc;
    CONC_HIP(hipDeviceSynchronize());
    m->n_seqs = d.n_seqs;
    m->view = conc_view{m->genes.p, m->gene_tx.p, m->tx.p, m->exons.p, m->expr.p, m->chrom_gene_first.p, m->chrom_genes.p, m->chrom_premax.p, m->names.p,
                        m->chrom_names.p, m->tx_names.p, m->seq_names.p, m->seq_sorted.p, m->chrom_seq.p, m->tx_seq.p, nullptr, (int32_t)d.n_chroms,
                        (int32_t)d.n_transcripts, (int32_t)d.n_seqs, 0};
    return DSA_OK;
}

int targets_run(conc_ctx* c, taskc_ctx* clusters, const conc_models* models, const task_reference* reference, int32_t range, conc_result* r)
{
    int ref_device = -1;
    const uint8_t* bytes = nullptr;
    const task_seq* seqs = nullptr;
    int64_t bytes_len = 0, n_seqs = 0;
    task_reference_device(reference, &ref_device, &bytes, &bytes_len, &seqs, &n_seqs);
    if (ref_device != c->device || models->device != c->device)
        return CONC_FAIL(DSA_E_ARG, "conc_targets: ctx, models and reference are on devices %d, %d and %d", c->device, models->device, ref_device);
    if (n_seqs != models->n_seqs) return CONC_FAIL(DSA_E_ARG, "conc_targets: the reference has %lld sequences, the models name %lld", (long long)n_seqs, (long long)models->n_seqs);
    CONC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    CONC_HIP(hipEventRecord(c->ev[0], st));
    // the groups: taskc_regions over the input, on the taskc_ctx's own stream (idle when it returns)
    taskc_result tr{};
    if (const int rc = taskc_regions(clusters, TASKC_INPUT, &tr)) return CONC_FAIL(rc, "conc_targets: taskc_regions: %s", taskc_last_error());
    r->n_lines = tr.n_lines;
    if (tr.stop_kind) {
        switch (tr.stop_kind) {                                 // (the regions rule over the input reports these three and no other)
        case TASKC_FEW_FIELDS: r->stop_kind = CONC_FEW_FIELDS; break;
        case TASKC_BAD_INTEGER: r->stop_kind = CONC_BAD_INTEGER; break;
        case TASKC_NOT_TWO_ENDS: r->stop_kind = CONC_NOT_TWO_ENDS; break;
        default: return CONC_FAIL(DSA_E_DEVICE, "internal: taskc_regions stopped with kind %d", tr.stop_kind);
        }
        r->stop_line = tr.stop_line;
        r->stop_field = tr.stop_field;
        r->stop_value = tr.stop_value;
        return DSA_OK;
    }
    if (tr.n_lines == 0) {
        c->lines = taskc_lines_view{};
        c->groups = taskc_groups_view{};
        c->n_clusters = c->n_targets = 0;
        c->has_targets = true;
        return DSA_OK;
    }
    if (const int rc = taskc_lines_device(clusters, false, &c->lines)) return CONC_FAIL(rc, "conc_targets: %s", taskc_last_error());
    if (const int rc = taskc_groups_device(clusters, &c->groups)) return CONC_FAIL(rc, "conc_targets: %s", taskc_last_error());
    const int64_t G = c->groups.n_groups;
    if (c->lines.device != c->device) return CONC_FAIL(DSA_E_ARG, "conc_targets: ctx and clusters are on devices %d and %d", c->device, c->lines.device);
    if (G < 1 || G > c->lines.n_input_lines) return CONC_FAIL(DSA_E_DEVICE, "internal: %lld groups of %lld lines", (long long)G, (long long)c->lines.n_input_lines);
    conc_view V = models->view;
    V.seqs = seqs;
    if (const int rc = reset_summary(c)) return rc;
    CONC_HIP(c->cnt.reserve((size_t)G));
    CONC_HIP(c->off.reserve((size_t)G));
    hipLaunchKernelGGL(k_targets<false>, dim3(grid_of(G)), dim3(BLOCK), 0, st, V, c->groups, c->lines, (int64_t)range, c->cnt.p, (const u64*)nullptr, (int64_t)0,
                       (conc_target*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, c->sum.p);
    CONC_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->cnt.p, c->off.p, (int)G, st); }));
    hipLaunchKernelGGL(k_total, dim3(1), dim3(64), 0, st, (const u64*)c->cnt.p, (const u64*)c->off.p, G, &c->sum.p->n_targets);
    if (const int rc = read_summary(c)) return rc;
    if (c->h_sum.stop != NO_STOP) {
        const int64_t g = (int64_t)(c->h_sum.stop >> 8);
        u64 key = 0;
        if (g >= G) return CONC_FAIL(DSA_E_DEVICE, "internal: a stop at group %lld of %lld", (long long)g, (long long)G);
        CONC_HIP(hipMemcpyAsync(&key, c->groups.key + g, sizeof key, hipMemcpyDeviceToHost, st));
        CONC_HIP(hipStreamSynchronize(st));
        r->stop_kind = (int32_t)(c->h_sum.stop & 0xFFu);
        r->stop_value = (int64_t)(int32_t)((uint32_t)(key >> 32) ^ SIGN);
        return DSA_OK;
    }
    // (behind the stops: the other end of an end on an empty sequence is a target on one)
    if (c->h_sum.limit) return CONC_FAIL(DSA_E_LIMIT, "conc_targets: a name of the form name:a-b, a coordinate beyond TASK_MAX_COORD or a target on an empty sequence");
    const int64_t n = (int64_t)c->h_sum.n_targets;
    if (n >= (int64_t)INT32_MAX) return CONC_FAIL(DSA_E_LIMIT, "conc_targets: %lld targets, more than 2^31 - 1", (long long)n);
    CONC_HIP(c->raw.reserve((size_t)n));
    CONC_HIP(c->tg.reserve((size_t)n));
    for (auto& b : c->key) CONC_HIP(b.reserve((size_t)n));
    for (auto& b : c->idx) CONC_HIP(b.reserve((size_t)n));
    if (n > 0) {
        hipLaunchKernelGGL(k_targets<true>, dim3(grid_of(G)), dim3(BLOCK), 0, st, V, c->groups, c->lines, (int64_t)range, (u64*)nullptr, (const u64*)c->off.p, n,
                           c->raw.p, c->key[0].p, c->idx[0].p, c->sum.p);
        CONC_HIP(hipEventRecord(c->ev[1], st));
        CONC_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->key[0].p, c->key[1].p, (const uint32_t*)c->idx[0].p, c->idx[1].p, (int)n, 0, 64, st);
        }));
        hipLaunchKernelGGL(k_permute, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const conc_target*)c->raw.p, (const uint32_t*)c->idx[1].p, n, c->tg.p);
    } else CONC_HIP(hipEventRecord(c->ev[1], st));
    CONC_HIP(hipEventRecord(c->ev[2], st));
    CONC_HIP(hipStreamSynchronize(st));
    CONC_HIP(hipGetLastError());
    c->timing.targets_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.sort_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->n_clusters = G / 2;
    c->n_targets = n;
    c->has_targets = true;
    r->n_clusters = c->n_clusters;
    r->n_targets = n;
    return DSA_OK;
}

int align_run(conc_ctx* c, const task_reference* reference, int32_t match, int32_t mismatch, int32_t gap, double threshold, conc_result* r)
{
    int ref_device = -1;
    const uint8_t* bytes = nullptr;
    const task_seq* seqs = nullptr;
    int64_t bytes_len = 0, n_seqs = 0;
    task_reference_device(reference, &ref_device, &bytes, &bytes_len, &seqs, &n_seqs);
    if (ref_device != c->device) return CONC_FAIL(DSA_E_ARG, "conc_align: ctx and reference are on devices %d and %d", c->device, ref_device);
    CONC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t n = c->n_targets;
    r->n_clusters = c->n_clusters;
    r->n_targets = n;
    c->timing.download_ms = c->timing.pack_ms = c->timing.dp_ms = 0.f;
    c->timing.cells = c->timing.n_packed16 = c->timing.n_int32 = 0;
    CONC_HIP(c->scores.reserve((size_t)n));
    if (n > 0) {
        CONC_HIP(c->pairs.reserve((size_t)n));
        std::vector<la_pair> pairs((size_t)n);
        std::vector<int32_t> need((size_t)n);
        CONC_HIP(hipEventRecord(c->ev[3], st));
        hipLaunchKernelGGL(k_pairs, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const conc_target*)c->tg.p, n, seqs, n_seqs, c->pairs.p);
        CONC_HIP(hipMemcpyAsync(pairs.data(), c->pairs.p, (size_t)n * sizeof(la_pair), hipMemcpyDeviceToHost, st));
        CONC_HIP(hipEventRecord(c->ev[4], st));
        CONC_HIP(hipStreamSynchronize(st));
        CONC_HIP(hipGetLastError());
        c->timing.download_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
        for (int64_t k = 0; k < n; ++k) need[(size_t)k] = threshold_min_score(score_max((size_t)pairs[(size_t)k].seq_len, match), threshold);
        la_timing lt{};
        if (const int rc = la_align_pairs_device(c->device, bytes, bytes_len, match, mismatch, gap, pairs.data(), n, need.data(), c->scores.p, &lt))
            return CONC_FAIL(rc, "conc_align: %s", la_last_error());
        c->timing.pack_ms = lt.pack_ms;
        c->timing.dp_ms = lt.kernel_ms;
        c->timing.cells = lt.cells;
        c->timing.n_packed16 = lt.n_packed16;
        c->timing.n_int32 = lt.n_int32;
    }
    c->match = match;
    c->threshold = threshold;
    c->has_scores = true;
    return DSA_OK;
}

int filter_run(conc_ctx* c, conc_result* r)
{
    CONC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t n = c->n_targets, m = c->lines.n_input_lines, K = c->n_clusters;
    r->n_lines = m;
    r->n_clusters = K;
    r->n_targets = n;
    if (m == 0) {
        c->align_bytes = c->out_bytes = 0;
        c->has_texts = true;
        return DSA_OK;
    }
    if (const int rc = reset_summary(c)) return rc;
    for (auto* b : {&c->alen, &c->adst}) CONC_HIP(b->reserve((size_t)n));
    for (auto* b : {&c->olen, &c->odst}) CONC_HIP(b->reserve((size_t)m));
    CONC_HIP(c->hit.reserve((size_t)K));
    CONC_HIP(hipEventRecord(c->ev[5], st));
    CONC_HIP(hipMemsetAsync(c->hit.p, 0, (size_t)K * sizeof(uint32_t), st));
    if (n > 0) {
        hipLaunchKernelGGL(k_decide, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const conc_target*)c->tg.p, (const int32_t*)c->scores.p, n, c->match, c->threshold,
                           c->groups, c->alen.p, c->hit.p, c->sum.p);
        CONC_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->alen.p, c->adst.p, (int)n, st); }));
    }
    hipLaunchKernelGGL(k_count_hits, dim3(grid_of(K)), dim3(BLOCK), 0, st, (const uint32_t*)c->hit.p, K, c->sum.p);
    hipLaunchKernelGGL(k_line_keep, dim3(grid_of(m)), dim3(BLOCK), 0, st, c->lines, c->groups, (const uint32_t*)c->hit.p, c->olen.p, c->sum.p);
    CONC_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->olen.p, c->odst.p, (int)m, st); }));
    hipLaunchKernelGGL(k_text_totals, dim3(1), dim3(64), 0, st, (const u64*)c->alen.p, (const u64*)c->adst.p, n, (const u64*)c->olen.p, (const u64*)c->odst.p, m,
                       c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    const Summary& s = c->h_sum;
    if (s.align_bytes < 0 || s.out_bytes < 0 || (int64_t)s.n_kept > n || (int64_t)s.n_kept_lines > m)
        return CONC_FAIL(DSA_E_DEVICE, "internal: %lld and %lld bytes of text", (long long)s.align_bytes, (long long)s.out_bytes);
    CONC_HIP(c->atext.reserve((size_t)s.align_bytes + 8));
    CONC_HIP(c->out.reserve((size_t)s.out_bytes + 8));
    if (n > 0)
        hipLaunchKernelGGL(k_print, dim3(grid_of(n)), dim3(BLOCK), 0, st, (const conc_target*)c->tg.p, (const int32_t*)c->scores.p, n, c->match,
                           (const u64*)c->alen.p, (const u64*)c->adst.p, c->atext.p, s.align_bytes);
    CONC_HIP(hipEventRecord(c->ev[6], st));
    hipLaunchKernelGGL(k_gather_lines<LINE_GROUP>, dim3(grid_of(m * LINE_GROUP)), dim3(BLOCK), 0, st, c->lines, (const u64*)c->olen.p, (const u64*)c->odst.p,
                       c->out.p, s.out_bytes);
    CONC_HIP(hipEventRecord(c->ev[7], st));
    CONC_HIP(hipStreamSynchronize(st));
    CONC_HIP(hipGetLastError());
    c->timing.print_ms = hiphost::elapsed(c->ev[5], c->ev[6]);
    c->timing.filter_ms = hiphost::elapsed(c->ev[6], c->ev[7]);
    c->align_bytes = s.align_bytes;
    c->out_bytes = s.out_bytes;
    c->has_texts = true;
    r->n_kept_targets = s.n_kept;
    r->align_bytes = s.align_bytes;
    r->n_hit_clusters = s.n_hit;
    r->n_kept_lines = s.n_kept_lines;
    r->out_bytes = s.out_bytes;
    r->n_noncanonical = s.n_noncanonical;
    return DSA_OK;
}

// what a failed or stopped stage leaves: nothing of it or of the stages behind it
void drop_from(conc_ctx* c, int stage)
{
    if (stage <= 0) {
        c->has_targets = false;
        c->n_targets = c->n_clusters = 0;
        c->lines = taskc_lines_view{};
        c->groups = taskc_groups_view{};
    }
    if (stage <= 1) c->has_scores = false;
    c->has_texts = false;
    c->align_bytes = c->out_bytes = 0;
}

}  // namespace

extern "C" {

const char* conc_last_error(void) { return g_conc_err.c_str(); }

int conc_models_create(int device, const conc_models_desc* desc, conc_models** out)
{
    if (!out) return CONC_FAIL(DSA_E_ARG, "conc_models_create: no output");
    *out = nullptr;
    if (!desc) return CONC_FAIL(DSA_E_ARG, "conc_models_create: no description");
    std::vector<int32_t> sorted;
    if (const int rc = check_models(*desc, sorted)) return rc;
    if (hiphost::check_device(device, &g_conc_err)) return DSA_E_DEVICE;
    CONC_HIP(hipSetDevice(device));
    conc_models* m = new conc_models();
    m->device = device;
    if (const int rc = build_models(m, *desc, sorted)) {
        delete m;
        return rc;
    }
    *out = m;
    return DSA_OK;
}

void conc_models_destroy(conc_models* m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

int conc_create(int device, conc_ctx** out)
{
    if (!out) return CONC_FAIL(DSA_E_ARG, "conc_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_conc_err)) return DSA_E_DEVICE;
    CONC_HIP(hipSetDevice(device));
    conc_ctx* c = new conc_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return CONC_FAIL(DSA_E_DEVICE, "conc_create: cannot create a stream or an event");
    }
    *out = c;
    return DSA_OK;
}

void conc_destroy(conc_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int conc_targets(conc_ctx* c, taskc_ctx* clusters, const conc_models* models, const task_reference* reference, int32_t range, conc_result* r)
{
    if (!r) return CONC_FAIL(DSA_E_ARG, "conc_targets: no result");
    clear_result(r);
    if (!c || !clusters || !models || !reference) return CONC_FAIL(DSA_E_ARG, "conc_targets: no %s", !c ? "ctx" : !clusters ? "clusters" : !models ? "models" : "reference");
    if (range < 0 || range > TASK_MAX_PARAM) return CONC_FAIL(DSA_E_LIMIT, "conc_targets: a range of %d, outside [0, TASK_MAX_PARAM]", range);
    drop_from(c, 0);
    c->timing = conc_timing{};
    const int rc = targets_run(c, clusters, models, reference, range, r);
    if (rc != DSA_OK || r->stop_kind) {
        (void)hipStreamSynchronize(c->st);
        drop_from(c, 0);
        if (rc != DSA_OK) clear_result(r);
    }
    return rc;
}

int conc_fetch_targets(conc_ctx* c, conc_target* out, int64_t n)
{
    if (!c) return CONC_FAIL(DSA_E_ARG, "conc_fetch_targets: no ctx");
    if (!c->has_targets) return CONC_FAIL(DSA_E_ARG, "conc_fetch_targets: the ctx has no targets (conc_targets first)");
    if (n != c->n_targets || (n && !out)) return CONC_FAIL(DSA_E_ARG, "conc_fetch_targets: room for %lld of %lld targets", (long long)n, (long long)c->n_targets);
    if (n == 0) return DSA_OK;
    CONC_HIP(hipSetDevice(c->device));
    CONC_HIP(hipMemcpyAsync(out, c->tg.p, (size_t)n * sizeof(conc_target), hipMemcpyDeviceToHost, c->st));
    CONC_HIP(hipStreamSynchronize(c->st));
    return DSA_OK;
}

int conc_align(conc_ctx* c, const task_reference* reference, int32_t match, int32_t mismatch, int32_t gap, double threshold, conc_result* r)
{
    if (!r) return CONC_FAIL(DSA_E_ARG, "conc_align: no result");
    clear_result(r);
    if (!c || !reference) return CONC_FAIL(DSA_E_ARG, "conc_align: no %s", !c ? "ctx" : "reference");
    if (match <= 0 || match > TASK_MAX_PARAM) return CONC_FAIL(DSA_E_ARG, "conc_align: a match score of %d, outside [1, TASK_MAX_PARAM]", match);
    if (!(threshold == threshold)) return CONC_FAIL(DSA_E_ARG, "conc_align: the threshold is no number");
    if (!c->has_targets) return CONC_FAIL(DSA_E_ARG, "conc_align: the ctx has no targets (conc_targets first)");
    drop_from(c, 1);
    const int rc = align_run(c, reference, match, mismatch, gap, threshold, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        drop_from(c, 1);
        clear_result(r);
    }
    return rc;
}

int conc_fetch_scores(conc_ctx* c, int32_t* out, int64_t n)
{
    if (!c) return CONC_FAIL(DSA_E_ARG, "conc_fetch_scores: no ctx");
    if (!c->has_scores) return CONC_FAIL(DSA_E_ARG, "conc_fetch_scores: the ctx has no scores (conc_align first)");
    if (n != c->n_targets || (n && !out)) return CONC_FAIL(DSA_E_ARG, "conc_fetch_scores: room for %lld of %lld scores", (long long)n, (long long)c->n_targets);
    if (n == 0) return DSA_OK;
    CONC_HIP(hipSetDevice(c->device));
    CONC_HIP(hipMemcpyAsync(out, c->scores.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
    CONC_HIP(hipStreamSynchronize(c->st));
    return DSA_OK;
}

int conc_filter(conc_ctx* c, conc_result* r)
{
    if (!r) return CONC_FAIL(DSA_E_ARG, "conc_filter: no result");
    clear_result(r);
    if (!c) return CONC_FAIL(DSA_E_ARG, "conc_filter: no ctx");
    if (!c->has_scores) return CONC_FAIL(DSA_E_ARG, "conc_filter: the ctx has no scores (conc_align first)");
    drop_from(c, 2);
    c->timing.print_ms = c->timing.filter_ms = 0.f;
    const int rc = filter_run(c, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        drop_from(c, 2);
        clear_result(r);
    }
    return rc;
}

int conc_fetch(conc_ctx* c, int32_t which, int64_t offset, uint8_t* buf, int64_t len)
{
    if (which != CONC_ALIGN_TEXT && which != CONC_FILTERED) return CONC_FAIL(DSA_E_ARG, "conc_fetch: which %d is neither CONC_ALIGN_TEXT nor CONC_FILTERED", which);
    if (!c) return CONC_FAIL(DSA_E_ARG, "conc_fetch: no ctx");
    if (!c->has_texts) return CONC_FAIL(DSA_E_ARG, "conc_fetch: the ctx has no texts (conc_filter first)");
    const int64_t bytes = which == CONC_ALIGN_TEXT ? c->align_bytes : c->out_bytes;
    if (offset < 0 || len < 0 || offset > bytes || len > bytes - offset)
        return CONC_FAIL(DSA_E_ARG, "conc_fetch: [%lld, +%lld) is outside the %lld bytes", (long long)offset, (long long)len, (long long)bytes);
    if (len && !buf) return CONC_FAIL(DSA_E_ARG, "conc_fetch: length without a buffer");
    if (len == 0) return DSA_OK;
    CONC_HIP(hipSetDevice(c->device));
    CONC_HIP(hipMemcpyAsync(buf, (which == CONC_ALIGN_TEXT ? c->atext.p : c->out.p) + offset, (size_t)len, hipMemcpyDeviceToHost, c->st));
    CONC_HIP(hipStreamSynchronize(c->st));
    return DSA_OK;
}

int conc_get_timing(const conc_ctx* c, conc_timing* out)
{
    if (!c || !out) return CONC_FAIL(DSA_E_ARG, "conc_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

int conc_into_taskc(const conc_ctx* c, taskc_ctx* into)
{
    if (!into || !c) return CONC_FAIL(DSA_E_ARG, "conc_into_taskc: no %s", !into ? "taskc_ctx" : "conc_ctx");
    if (!c->has_texts) return CONC_FAIL(DSA_E_ARG, "conc_into_taskc: the ctx has no filtered text (conc_filter first)");
    const int rc = taskc_add_device(into, c->device, c->out.p, c->out_bytes);      // (conc_filter returned: its stream is idle)
    if (rc != DSA_OK) return CONC_FAIL(rc, "conc_into_taskc: %s", taskc_last_error());
    return DSA_OK;
}

}  // extern "C"
