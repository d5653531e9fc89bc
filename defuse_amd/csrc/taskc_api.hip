// taskc_api.hip — remove_duplicates and get_align_regions on cluster text in device memory, for gfx950 (include/defuse_task.h,
// section "cluster text"): the two host steps of bin/defuse_glue between sct_cover and taskt_parse_regions.
//
// Text: every piece (taskc_add from the host, taskc_add_cover from an sct_ctx's output) is appended to one device buffer at a
// 16-byte boundary, its newlines are found by the table kernels of txt_shared.hpp, and k_piece_lines appends the 64-bit start and
// the length of each of its lines to the per-line arrays.  Nothing later knows of pieces; the host keeps their places to turn a
// stopping line into an offset of the caller's input.
// Parse (once per input, for both steps): k_parse, one lane per line through taskc_shared.hpp.
// Dedup, over the lines in front of the first line stop:
//   runs     k_run_heads compares each id with the line in front (piece boundaries are not seen), an inclusive sum numbers the runs
//   sorts    a stable 2-bit radix sort by cluster end (lines without a fragment go last), then a stable sort by (run, fragment
//            with the sign bit turned): a fragment's end-0 lines, then its end-1 lines, each in file order, fragments ascending.
//            The last line of each (fragment, end) wins; a fragment without a winner on either side is the missing end
//   select   a stable sort of the fragments by position 1, then by (run, position 0): equal pairs side by side, the lowest
//            fragment first, which is kept.  The kept counts of a run are the difference of an inclusive sum at its two edges
//   output   per fragment in (run, fragment) order its two lines' lengths, a 64-bit exclusive sum, and k_gather: 16 lanes copy
//            one line dword by dword (bat_shared.hpp's scheme) and one of them stores the newline
// Regions, over the input's lines or the dedup text's (which are input lines: their parsed records are reused):
//   a stable sort by (id, cluster end), both with the sign bit turned; heads and an inclusive sum number the groups; the least
//   start and greatest end by two reductions by key, name and strand from the group's last line; the ends of every id are
//   counted on the groups' keys; lengths, a 64-bit exclusive sum, and k_region_print with 16 lanes per group.
// Every read of the text is inside a line or inside the zeroed padding behind the last piece; every per-line array is indexed
// below the number of lines, every per-fragment array below the number of fragment lines, every store into an output lies inside
// the bytes its scan counted.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_task.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "taskc_shared.hpp"
#include "txt_shared.hpp"

// sct_api.hip, taskt_api.hip
__attribute__((visibility("hidden"))) bool sct_cover_output_device(const sct_ctx* c, int* device, const uint8_t** text, int64_t* len);
__attribute__((visibility("hidden"))) int taskt_regions_from_device(taskt_ctx* c, const taskt_names* seq_names, int device, const uint8_t* text, int64_t len,
                                                                    taskt_result* result);

namespace {

using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using hiphost::grow_keep;
using hiphost::Keep;

thread_local std::string g_taskc_err;

#define TASKC_HIP(call) HIPHOST_TRY(g_taskc_err, call)
#define TASKC_FAIL(code, ...) hiphost::fail(g_taskc_err, code, __VA_ARGS__)

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t SIGN = 0x80000000u;        // int order as unsigned order
constexpr int LINE_GROUP = 16;                // lanes per copied line and per printed region
static_assert(TEXT_PAD >= batdev::SRC_PAD + CHUNK, "padding");        // k_gather reads the text; the padding lies behind the last piece
static_assert(sizeof(taskc_result) == 96 && sizeof(taskc_timing) == 48 && sizeof(taskc_line) == 44, "layout");

// what the host reads between the stages (in: the stops NONE, the counts 0)
struct Summary {
    uint32_t dstop, rstop;      // the lowest line stopped by the dedup / the regions rule
    uint32_t n_frag_lines;      // lines with cluster end 0 or 1
    uint32_t n_runs, n_frags;
    uint32_t miss;              // the lowest fragment (in (run, fragment) order) without one of its ends
    uint32_t bad_group;         // the lowest group that begins an id without exactly two ends
    uint32_t n_groups, n_ids;
    uint32_t pad_;
    u64 n_kept_frags, n_kept_runs;
    int64_t out_bytes;
};

// ---- text ------------------------------------------------------------------------------------------------------------

// line j of a piece at `base` of the buffer: where it starts and how long it is
__global__ __launch_bounds__(BLOCK) void k_piece_lines(const uint32_t* __restrict__ nl_pos, int64_t n_nl, int64_t n_lines, int64_t base, int64_t len,
                                                        int64_t* __restrict__ lstart, int32_t* __restrict__ llen)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_lines) return;
    const int64_t s = j == 0 ? 0 : (int64_t)nl_pos[j - 1] + 1;
    const int64_t e = j < n_nl ? (int64_t)nl_pos[j] : len;
    lstart[j] = base + s;
    llen[j] = (int32_t)(e - s);
}

__global__ __launch_bounds__(BLOCK) void k_parse(const uint8_t* __restrict__ text, const int64_t* __restrict__ lstart, const int32_t* __restrict__ llen, int64_t n,
                                                  taskc_line* __restrict__ rec, Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t s = lstart[i];
    const taskc_line r = taskc_parse_line(text, s, s + (int64_t)llen[i], DeviceInt());
    rec[i] = r;
    if (r.dkind) atomicMin(&sum->dstop, (uint32_t)i);           // (rare)
    if (r.rkind) atomicMin(&sum->rstop, (uint32_t)i);
}

// ---- dedup -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void k_run_heads(const taskc_line* __restrict__ rec, int64_t m, uint32_t* __restrict__ head, uint32_t* __restrict__ key,
                                                      uint32_t* __restrict__ idx, Summary* __restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t carries = 0;
    if (i < m) {
        const int32_t ce = rec[i].ce;
        carries = (ce == 0 || ce == 1) ? 1u : 0u;
        head[i] = (i == 0 || rec[i].id != rec[i - 1].id) ? 1u : 0u;
        key[i] = carries ? (uint32_t)ce : 2u;
        idx[i] = (uint32_t)i;
    }
    const uint32_t n = Reduce(tmp).Sum(carries);                // (every lane of the workgroup is here)
    if (threadIdx.x == 0 && n) atomicAdd(&sum->n_frag_lines, n);
}

// run_first[r] = the first line of run r; run_first[n_runs] = m
__global__ __launch_bounds__(BLOCK) void k_run_first(const uint32_t* __restrict__ head, const uint32_t* __restrict__ runp, int64_t m, uint32_t* __restrict__ run_first,
                                                      Summary* __restrict__ sum)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    if (head[i]) run_first[runp[i] - 1] = (uint32_t)i;          // runp[i] in [1, m]
    if (i == m - 1) {
        run_first[runp[i]] = (uint32_t)m;
        sum->n_runs = runp[i];
    }
}

__global__ __launch_bounds__(BLOCK) void k_frag_keys(const uint32_t* __restrict__ idx, const taskc_line* __restrict__ rec, const uint32_t* __restrict__ runp, int64_t F,
                                                      int64_t m, u64* __restrict__ key)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= F) return;
    const int64_t i = idx[s];
    key[s] = i < m ? ((u64)(runp[i] - 1) << 32) | (u64)((uint32_t)rec[i].frag ^ SIGN) : 0ull;
}

__global__ __launch_bounds__(BLOCK) void k_key_heads(const u64* __restrict__ key, int64_t n, uint32_t* __restrict__ head)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n) head[s] = (s == 0 || key[s] != key[s - 1]) ? 1u : 0u;
}

// the last line of every (fragment, end) at its place in win[2 * fragment + end] (in: NONE); the fragment's (run, fragment) key
__global__ __launch_bounds__(BLOCK) void k_winners(const u64* __restrict__ key, const uint32_t* __restrict__ idx, const taskc_line* __restrict__ rec,
                                                    const uint32_t* __restrict__ fp, int64_t F, int64_t m, uint32_t* __restrict__ win, u64* __restrict__ fkey,
                                                    Summary* __restrict__ sum)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= F) return;
    const int64_t i = idx[s], j = (int64_t)fp[s] - 1;            // j in [0, F)
    if (s == F - 1) sum->n_frags = fp[s];
    if (i >= m || j < 0 || j >= F) return;
    const int32_t ce = rec[i].ce & 1;
    const bool last = s + 1 == F || key[s + 1] != key[s] || (idx[s + 1] < m && (rec[idx[s + 1]].ce & 1) != ce);
    if (last) win[2 * j + ce] = (uint32_t)i;
    if (s == 0 || key[s] != key[s - 1]) fkey[j] = key[s];
}

// a fragment of a run other than skip_run that lacks an end; the positions of the others, and the first sort's keys
__global__ __launch_bounds__(BLOCK) void k_frag_pos(const uint32_t* __restrict__ win, const u64* __restrict__ fkey, const taskc_line* __restrict__ rec, int64_t nf,
                                                     int64_t m, uint32_t skip_run, int32_t* __restrict__ p0, int32_t* __restrict__ p1, uint32_t* __restrict__ key,
                                                     uint32_t* __restrict__ fidx, Summary* __restrict__ sum)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nf) return;
    const uint32_t a = win[2 * j], b = win[2 * j + 1];
    int32_t x = 0, y = 0;
    if (a >= m || b >= m) {
        if ((uint32_t)(fkey[j] >> 32) != skip_run) atomicMin(&sum->miss, (uint32_t)j);      // (rare)
    } else {
        x = rec[a].pos;
        y = rec[b].pos;
    }
    p0[j] = x;
    p1[j] = y;
    key[j] = (uint32_t)y ^ SIGN;
    fidx[j] = (uint32_t)j;
}

__global__ __launch_bounds__(BLOCK) void k_pos_keys(const uint32_t* __restrict__ fidx, const u64* __restrict__ fkey, const int32_t* __restrict__ p0, int64_t nf,
                                                     u64* __restrict__ key)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nf) return;
    const int64_t j = fidx[t];
    key[t] = j < nf ? (fkey[j] & 0xFFFFFFFF00000000ull) | (u64)((uint32_t)p0[j] ^ SIGN) : 0ull;
}

// the first fragment of every distinct (run, position 0, position 1)
__global__ __launch_bounds__(BLOCK) void k_dup_heads(const u64* __restrict__ key, const uint32_t* __restrict__ fidx, const int32_t* __restrict__ p1, int64_t nf,
                                                      uint32_t* __restrict__ hd, uint32_t* __restrict__ keepf)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nf) return;
    const int64_t j = fidx[t];
    if (j >= nf) return;
    uint32_t h = 1;
    if (t > 0) {
        const int64_t q = fidx[t - 1];
        h = (key[t] != key[t - 1] || (q < nf && p1[q] != p1[j])) ? 1u : 0u;
    }
    hd[t] = h;
    keepf[j] = h;
}

// the inclusive sum of the heads at the two edges of every run's fragments (runs without a fragment keep their zeros)
__global__ __launch_bounds__(BLOCK) void k_run_edges(const u64* __restrict__ key, const uint32_t* __restrict__ hd, const uint32_t* __restrict__ hp, int64_t nf,
                                                      int64_t n_runs, uint32_t* __restrict__ rlo, uint32_t* __restrict__ rhi)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nf) return;
    const int64_t r = (int64_t)(key[t] >> 32);
    if (r >= n_runs) return;
    if (t == 0 || (int64_t)(key[t - 1] >> 32) != r) rlo[r] = hp[t] - hd[t];
    if (t == nf - 1 || (int64_t)(key[t + 1] >> 32) != r) rhi[r] = hp[t];
}

__global__ __launch_bounds__(BLOCK) void k_runs_kept(const uint32_t* __restrict__ rlo, const uint32_t* __restrict__ rhi, int64_t n_runs, int64_t min_size,
                                                      Summary* __restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t k = (r < n_runs && (int64_t)(rhi[r] - rlo[r]) >= min_size) ? 1u : 0u;
    const uint32_t n = Reduce(tmp).Sum(k);
    if (threadIdx.x == 0 && n) atomicAdd(&sum->n_kept_runs, (u64)n);
}

// per fragment in (run, fragment) order: printed or not, and the bytes of its two lines
__global__ __launch_bounds__(BLOCK) void k_frag_out(const u64* __restrict__ fkey, const uint32_t* __restrict__ keepf, const uint32_t* __restrict__ rlo,
                                                     const uint32_t* __restrict__ rhi, const uint32_t* __restrict__ win, const int32_t* __restrict__ llen, int64_t nf,
                                                     int64_t n_runs, int64_t m, int64_t min_size, uint32_t* __restrict__ of, u64* __restrict__ flen)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nf) return;
    const int64_t r = (int64_t)(fkey[j] >> 32);
    const uint32_t a = win[2 * j], b = win[2 * j + 1];
    const bool out = keepf[j] && r < n_runs && (int64_t)(rhi[r] - rlo[r]) >= min_size && a < m && b < m;
    of[j] = out ? 1u : 0u;
    flen[j] = out ? (u64)llen[a] + (u64)llen[b] + 2ull : 0ull;
}

// the two output lines of every printed fragment: their input lines and their places; the totals
__global__ __launch_bounds__(BLOCK) void k_out_lines(const uint32_t* __restrict__ of, const uint32_t* __restrict__ orank, const u64* __restrict__ flen,
                                                      const u64* __restrict__ fdst, const uint32_t* __restrict__ win, const int32_t* __restrict__ llen, int64_t nf,
                                                      uint32_t* __restrict__ osrc, u64* __restrict__ odst, Summary* __restrict__ sum)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nf) return;
    if (j == nf - 1) {
        sum->n_kept_frags = (u64)orank[j] + (u64)of[j];
        sum->out_bytes = (int64_t)(fdst[j] + flen[j]);
    }
    if (!of[j]) return;
    const int64_t k = 2 * (int64_t)orank[j];                    // below 2 nf
    const uint32_t a = win[2 * j], b = win[2 * j + 1];
    osrc[k] = a;
    osrc[k + 1] = b;
    odst[k] = fdst[j];
    odst[k + 1] = fdst[j] + (u64)llen[a] + 1ull;
}

// k_bat_gather's scheme with a line per group of G lanes, which copy it by copy_span; the first lane that has no head or tail
// byte of the line stores the newline.
template <int G>
__global__ __launch_bounds__(BLOCK) void k_gather(const uint32_t* __restrict__ osrc, const u64* __restrict__ odst, int64_t n_out, const uint8_t* __restrict__ text,
                                                   int64_t text_len, const int64_t* __restrict__ lstart, const int32_t* __restrict__ llen, int64_t m,
                                                   uint8_t* __restrict__ dst, int64_t dst_len)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t k = t / G;
    const int lane = (int)(t % G);
    if (k >= n_out) return;
    const int64_t i = osrc[k];
    if (i >= m) return;
    const int64_t src = lstart[i], len = llen[i];
    const int64_t d0 = (int64_t)odst[k], d1 = d0 + len;
    if (d0 < 0 || d1 + 1 > dst_len || src < 0 || src + len > text_len) return;
    const int64_t n_edge = copy_span<G>(text, src, dst, d0, len, lane);       // at most six
    if (G - 1 - lane == n_edge) dst[d1] = '\n';
}

// ---- regions ---------------------------------------------------------------------------------------------------------

// item k of the source is the input line src[k] (src NULL: k itself)
__device__ inline int64_t source_line(const uint32_t* __restrict__ src, int64_t k) { return src ? (int64_t)src[k] : k; }

__global__ __launch_bounds__(BLOCK) void k_region_keys(const taskc_line* __restrict__ rec, const uint32_t* __restrict__ src, int64_t q, int64_t m,
                                                        u64* __restrict__ key, uint32_t* __restrict__ idx, Summary* __restrict__ sum)
{
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= q) return;
    const int64_t i = source_line(src, k);
    u64 v = 0;
    if (i < m) {
        const taskc_line r = rec[i];
        v = ((u64)((uint32_t)r.id ^ SIGN) << 32) | (u64)((uint32_t)r.ce ^ SIGN);
        if (r.rkind) atomicMin(&sum->rstop, (uint32_t)k);       // (rare)
    }
    key[k] = v;
    idx[k] = (uint32_t)k;
}

// after the sort: every item's start and end, and the group's last line at the group's number
__global__ __launch_bounds__(BLOCK) void k_region_vals(const u64* __restrict__ key, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ gp,
                                                        const taskc_line* __restrict__ rec, const uint32_t* __restrict__ src, int64_t q, int64_t m,
                                                        int32_t* __restrict__ vstart, int32_t* __restrict__ vend, uint32_t* __restrict__ glast,
                                                        Summary* __restrict__ sum)
{
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= q) return;
    const int64_t k = idx[s];
    const int64_t i = k < q ? source_line(src, k) : m;
    vstart[s] = i < m ? rec[i].start : 0;
    vend[s] = i < m ? rec[i].end : 0;
    if (s == q - 1) sum->n_groups = gp[s];
    if (s + 1 == q || key[s + 1] != key[s]) glast[gp[s] - 1] = (uint32_t)i;      // gp[s] in [1, q]
}

// on the groups' keys: an id whose first group is not followed by exactly one more of it; the ids counted; every group's bytes
__global__ __launch_bounds__(BLOCK) void k_region_groups(const u64* __restrict__ gkey, const int32_t* __restrict__ gmin, const int32_t* __restrict__ gmax,
                                                          const uint32_t* __restrict__ glast, const taskc_line* __restrict__ rec, int64_t q, int64_t m,
                                                          u64* __restrict__ glen, Summary* __restrict__ sum)
{
    using Reduce = hipcub::BlockReduce<uint32_t, BLOCK>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t G = sum->n_groups;                             // (written by the kernel in front)
    uint32_t first = 0;
    if (g < q) {
        u64 bytes = 0;
        if (g < G) {
            const uint32_t id = (uint32_t)(gkey[g] >> 32);
            first = (g == 0 || (uint32_t)(gkey[g - 1] >> 32) != id) ? 1u : 0u;
            if (first) {
                const bool two = g + 1 < G && (uint32_t)(gkey[g + 1] >> 32) == id && (g + 2 >= G || (uint32_t)(gkey[g + 2] >> 32) != id);
                if (!two) atomicMin(&sum->bad_group, (uint32_t)g);
            }
            const int64_t i = glast[g];
            if (i < m)
                bytes = (u64)(taskc_dec_len((int32_t)(id ^ SIGN)) + taskc_dec_len((int32_t)((uint32_t)gkey[g] ^ SIGN)) + rec[i].name_len + rec[i].strand_len +
                              taskc_dec_len(gmin[g]) + taskc_dec_len(gmax[g]) + 6);
        }
        glen[g] = bytes;
    }
    const uint32_t n = Reduce(tmp).Sum(first);
    if (threadIdx.x == 0 && n) atomicAdd(&sum->n_ids, n);
}

__global__ void k_region_total(const u64* __restrict__ glen, const u64* __restrict__ gdst, int64_t q, Summary* __restrict__ sum)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) sum->out_bytes = (int64_t)(gdst[q - 1] + glen[q - 1]);
}

// G lanes per group: lanes 0-3 write one integer each and the byte behind it, all of them copy the name and the strand
template <int G>
__global__ __launch_bounds__(BLOCK) void k_region_print(const u64* __restrict__ gkey, const int32_t* __restrict__ gmin, const int32_t* __restrict__ gmax,
                                                         const uint32_t* __restrict__ glast, const u64* __restrict__ gdst, const u64* __restrict__ glen,
                                                         const taskc_line* __restrict__ rec, const uint8_t* __restrict__ text, const int64_t* __restrict__ lstart,
                                                         int64_t n_groups, int64_t m, uint8_t* __restrict__ out, int64_t out_len)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int64_t g = t / G;
    const int lane = (int)(t % G);
    if (g >= n_groups) return;
    const int64_t i = glast[g];
    const int64_t d = (int64_t)gdst[g];
    if (i >= m || d < 0 || d + (int64_t)glen[g] > out_len || glen[g] == 0) return;
    const taskc_line r = rec[i];
    const int32_t v[4] = {(int32_t)((uint32_t)(gkey[g] >> 32) ^ SIGN), (int32_t)((uint32_t)gkey[g] ^ SIGN), gmin[g], gmax[g]};
    const int64_t at_ce = d + taskc_dec_len(v[0]) + 1;
    const int64_t at_name = at_ce + taskc_dec_len(v[1]) + 1;
    const int64_t at_strand = at_name + r.name_len + 1;
    const int64_t at_start = at_strand + r.strand_len + 1;
    const int64_t at_end = at_start + taskc_dec_len(v[2]) + 1;
    const uint8_t* __restrict__ line = text + lstart[i];
    for (int32_t b = lane; b < r.name_len; b += G) out[at_name + b] = line[r.name_off + b];
    for (int32_t b = lane; b < r.strand_len; b += G) out[at_strand + b] = line[r.strand_off + b];
    if (lane < 4) {
        const int64_t at = lane == 0 ? d : lane == 1 ? at_ce : lane == 2 ? at_start : at_end;
        const int n = taskc_dec_put(lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : v[3], out + at);
        out[at + n] = lane == 3 ? '\n' : '\t';
    } else if (lane == 4) out[at_strand - 1] = '\t';
    else if (lane == 5) out[at_start - 1] = '\t';
}

struct Piece {                  // host: where a piece lies
    int64_t buf_base, in_base, len, line_base, n_lines;
};

int bits_for(int64_t max_value)
{
    int bits = 1;
    while ((1ll << bits) <= max_value) ++bits;
    return bits;
}

}  // namespace

struct taskc_ctx {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[12];      // 0-2 a piece; 3, 4 parse; 5-8 dedup; 9-11 regions
    taskc_timing timing{};
    // the text and its lines
    DeviceBuffer<uint8_t> text;
    DeviceBuffer<int64_t> lstart;
    DeviceBuffer<int32_t> llen;
    std::vector<Piece> pieces;
    int64_t text_used = 0, n_lines = 0, n_bytes = 0;
    // scratch of a piece's tables
    TextScratch scratch;
    DeviceBuffer<uint32_t, GrowSize> nl_pos;
    // the parsed lines
    DeviceBuffer<taskc_line, GrowSize> rec;
    DeviceBuffer<Summary> sum;
    Summary h_sum{};
    bool parsed = false;
    uint32_t dstop = NONE;
    // scratch of both steps
    DeviceBuffer<uint32_t, GrowSize> head, runp, run_first, k32[2], idx[2], fp, win, keepf, hd, hp, rlo, rhi, of, orank, glast;
    DeviceBuffer<u64, GrowSize> k64[2], fkey, flen, fdst, glen, gdst;
    DeviceBuffer<int32_t, GrowSize> p0, p1, vstart, vend, gmin, gmax;
    DeviceBuffer<uint32_t> n_unique;
    // the dedup text: its bytes, and per line the input line and the offset
    DeviceBuffer<uint8_t, GrowSize> dout;
    DeviceBuffer<uint32_t, GrowSize> osrc;
    DeviceBuffer<u64, GrowSize> odst;
    int64_t dout_bytes = 0, dout_lines = 0;
    bool has_dedup = false;
    // the regions text
    DeviceBuffer<uint8_t, GrowSize> rout;
    int64_t rout_bytes = 0;
    bool has_regions = false;
    int64_t n_groups = 0;       // of the regions text, -1 if it is the dedup text's
    // small device-to-host copies land here
    u64 h_u64 = 0;
    uint32_t h_u32 = 0;
    int64_t h_lstart = 0;
    int32_t h_llen = 0;
};

namespace {

void drop_outputs(taskc_ctx* c)
{
    c->has_dedup = c->has_regions = c->parsed = false;
    c->dout_bytes = c->dout_lines = c->rout_bytes = 0;
    c->dstop = NONE;
    c->timing.parse_ms = 0.f;
}

// One piece (len > 0) behind the text, from host memory or from this device's.
int add_piece(taskc_ctx* c, const uint8_t* src, int64_t len, hipMemcpyKind kind)
{
    TASKC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t base = c->text_used;
    TASKC_HIP(grow_keep(c->text, Keep{(size_t)base}, (size_t)base + padded_size(len), st));
    uint8_t* at = c->text.p + base;
    Totals tot{};
    if (const int rc = text_upload_count<false>(g_taskc_err, c->scratch, at, src, kind, len, c->ev[0], c->ev[1], st, tot)) return rc;
    const int64_t n_nl = (int64_t)tot.n_nl;
    const int64_t n_lines = n_nl + (tot.last != '\n' ? 1 : 0);
    if (c->n_lines + n_lines > (int64_t)INT32_MAX) return TASKC_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 cluster lines");
    TASKC_HIP(c->nl_pos.reserve((size_t)n_nl));
    TASKC_HIP(grow_keep(c->lstart, Keep{(size_t)c->n_lines}, (size_t)(c->n_lines + n_lines), st));
    TASKC_HIP(grow_keep(c->llen, Keep{(size_t)c->n_lines}, (size_t)(c->n_lines + n_lines), st));
    text_place_tables<false>(c->scratch, at, len, tot, c->nl_pos.p, nullptr, nullptr, st);
    hipLaunchKernelGGL(k_piece_lines, dim3(grid_of(n_lines)), dim3(BLOCK), 0, st, (const uint32_t*)c->nl_pos.p, n_nl, n_lines, base, len, c->lstart.p + c->n_lines,
                       c->llen.p + c->n_lines);
    TASKC_HIP(hipEventRecord(c->ev[2], st));
    TASKC_HIP(hipStreamSynchronize(st));
    TASKC_HIP(hipGetLastError());
    c->pieces.push_back(Piece{base, c->n_bytes, len, c->n_lines, n_lines});
    c->text_used = base + chunks_of(len) * CHUNK;
    c->n_lines += n_lines;
    c->n_bytes += len;
    c->timing.upload_ms += hiphost::elapsed(c->ev[0], c->ev[1]);
    c->timing.tables_ms += hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.text_bytes = c->n_bytes;
    c->timing.n_pieces = (int64_t)c->pieces.size();
    return DSA_OK;
}

int reset_summary(taskc_ctx* c)
{
    TASKC_HIP(c->sum.reserve(1));
    c->h_sum = Summary{};
    c->h_sum.dstop = c->h_sum.rstop = c->h_sum.miss = c->h_sum.bad_group = NONE;
    TASKC_HIP(hipMemcpyAsync(c->sum.p, &c->h_sum, sizeof(Summary), hipMemcpyHostToDevice, c->st));
    return DSA_OK;
}

int read_summary(taskc_ctx* c)
{
    TASKC_HIP(hipMemcpyAsync(&c->h_sum, c->sum.p, sizeof(Summary), hipMemcpyDeviceToHost, c->st));
    TASKC_HIP(hipStreamSynchronize(c->st));
    TASKC_HIP(hipGetLastError());
    return DSA_OK;
}

// The line rule over the whole input, once.
int ensure_parsed(taskc_ctx* c)
{
    if (c->parsed || c->n_lines == 0) return DSA_OK;
    hipStream_t st = c->st;
    TASKC_HIP(c->rec.reserve((size_t)c->n_lines));
    if (const int rc = reset_summary(c)) return rc;
    TASKC_HIP(hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL(k_parse, dim3(grid_of(c->n_lines)), dim3(BLOCK), 0, st, (const uint8_t*)c->text.p, (const int64_t*)c->lstart.p, (const int32_t*)c->llen.p,
                       c->n_lines, c->rec.p, c->sum.p);
    TASKC_HIP(hipEventRecord(c->ev[4], st));
    if (const int rc = read_summary(c)) return rc;
    c->timing.parse_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    c->dstop = c->h_sum.dstop;
    c->parsed = true;
    return DSA_OK;
}

// The stop at input line g (0-based): its place in the caller's input, kind and field by `dedup` or the regions rule.
int line_stop(taskc_ctx* c, int64_t g, bool dedup, int kind, int64_t value, taskc_result* r)
{
    hipStream_t st = c->st;
    taskc_line rec{};
    TASKC_HIP(hipMemcpyAsync(&c->h_lstart, c->lstart.p + g, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    TASKC_HIP(hipMemcpyAsync(&c->h_llen, c->llen.p + g, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TASKC_HIP(hipMemcpyAsync(&rec, c->rec.p + g, sizeof rec, hipMemcpyDeviceToHost, st));
    TASKC_HIP(hipStreamSynchronize(st));
    size_t p = c->pieces.size() - 1;
    while (p > 0 && c->pieces[p].line_base > g) --p;
    const Piece& pc = c->pieces[p];
    r->stop_line = g + 1;
    r->stop_off = c->h_lstart - pc.buf_base + pc.in_base;
    r->stop_len = c->h_llen;
    r->stop_kind = kind ? kind : dedup ? rec.dkind : rec.rkind;
    r->stop_field = kind ? -1 : dedup ? rec.dfield : rec.rfield;
    r->stop_value = value;
    if (r->stop_kind <= 0 || r->stop_off < 0 || r->stop_off + r->stop_len > c->n_bytes)
        return TASKC_FAIL(DSA_E_DEVICE, "internal: a stop at line %lld that is none", (long long)(g + 1));
    return DSA_OK;
}

int dedup_run(taskc_ctx* c, int64_t min_size, taskc_result* r)
{
    TASKC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t n = c->n_lines;
    r->n_lines = n;
    if (n == 0) return DSA_OK;
    const bool parsed_before = c->parsed;                       // (else the parse lies between the two events below)
    TASKC_HIP(hipEventRecord(c->ev[5], st));
    if (const int rc = ensure_parsed(c)) return rc;
    // The lines in front of the first line stop L are looked at.  If L stopped on its position field it belongs to its run: if
    // that is the run of the line in front, that run is open, and what it lacks is not reported (its last line is L or behind).
    const bool stopped = (int64_t)c->dstop < n;
    const int64_t m = stopped ? (int64_t)c->dstop : n;
    bool open_tail = false;
    if (stopped && m > 0) {
        taskc_line two[2];
        TASKC_HIP(hipMemcpyAsync(two, c->rec.p + (m - 1), sizeof two, hipMemcpyDeviceToHost, st));
        TASKC_HIP(hipStreamSynchronize(st));
        open_tail = two[1].dkind == TASKC_BAD_INTEGER && two[1].dfield >= 6 && two[1].id == two[0].id;
    }
    if (m == 0) return line_stop(c, 0, true, 0, 0, r);
    if (const int rc = reset_summary(c)) return rc;
    Summary& sum = c->h_sum;

    // runs, and the order by cluster end
    for (auto* b : {&c->head, &c->runp, &c->k32[0], &c->k32[1], &c->idx[0], &c->idx[1]}) TASKC_HIP(b->reserve((size_t)m));
    TASKC_HIP(c->run_first.reserve((size_t)m + 1));
    hipLaunchKernelGGL(k_run_heads, dim3(grid_of(m)), dim3(BLOCK), 0, st, (const taskc_line*)c->rec.p, m, c->head.p, c->k32[0].p, c->idx[0].p, c->sum.p);
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->head.p, c->runp.p, (int)m, st); }));
    hipLaunchKernelGGL(k_run_first, dim3(grid_of(m)), dim3(BLOCK), 0, st, (const uint32_t*)c->head.p, (const uint32_t*)c->runp.p, m, c->run_first.p, c->sum.p);
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, (const uint32_t*)c->k32[0].p, c->k32[1].p, (const uint32_t*)c->idx[0].p, c->idx[1].p, (int)m, 0, 2, st);
    }));
    if (const int rc = read_summary(c)) return rc;
    const int64_t F = sum.n_frag_lines, n_runs = sum.n_runs;
    if (F > m || n_runs < 1 || n_runs > m) return TASKC_FAIL(DSA_E_DEVICE, "internal: %lld fragment lines and %lld runs in %lld lines", (long long)F, (long long)n_runs, (long long)m);

    // fragments: the order by (run, fragment), the winners, the missing ends
    int64_t nf = 0;
    if (F) {
        for (auto* b : {&c->k64[0], &c->k64[1], &c->fkey}) TASKC_HIP(b->reserve((size_t)F));
        for (auto* b : {&c->fp, &c->hd}) TASKC_HIP(b->reserve((size_t)F));
        TASKC_HIP(c->win.reserve(2 * (size_t)F));
        hipLaunchKernelGGL(k_frag_keys, dim3(grid_of(F)), dim3(BLOCK), 0, st, (const uint32_t*)c->idx[1].p, (const taskc_line*)c->rec.p, (const uint32_t*)c->runp.p, F, m,
                           c->k64[0].p);
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->k64[0].p, c->k64[1].p, (const uint32_t*)c->idx[1].p, c->idx[0].p, (int)F, 0,
                                                      32 + bits_for(n_runs - 1), st);
        }));
        hipLaunchKernelGGL(k_key_heads, dim3(grid_of(F)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, F, c->hd.p);
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->hd.p, c->fp.p, (int)F, st); }));
        TASKC_HIP(hipMemsetAsync(c->win.p, 0xFF, 2 * (size_t)F * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_winners, dim3(grid_of(F)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, (const uint32_t*)c->idx[0].p, (const taskc_line*)c->rec.p,
                           (const uint32_t*)c->fp.p, F, m, c->win.p, c->fkey.p, c->sum.p);
        // (at most F fragments: the per-fragment arrays are sized by F and the kernels launched over the count the host reads next)
        for (auto* b : {&c->p0, &c->p1}) TASKC_HIP(b->reserve((size_t)F));
        for (auto* b : {&c->keepf, &c->hp, &c->of, &c->orank}) TASKC_HIP(b->reserve((size_t)F));
        for (auto* b : {&c->flen, &c->fdst}) TASKC_HIP(b->reserve((size_t)F));
        if (const int rc = read_summary(c)) return rc;
        nf = sum.n_frags;
        if (nf < 1 || nf > F) return TASKC_FAIL(DSA_E_DEVICE, "internal: %lld fragments of %lld lines", (long long)nf, (long long)F);
        hipLaunchKernelGGL(k_frag_pos, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const uint32_t*)c->win.p, (const u64*)c->fkey.p, (const taskc_line*)c->rec.p, nf, m,
                           open_tail ? (uint32_t)(n_runs - 1) : NONE, c->p0.p, c->p1.p, c->k32[0].p, c->idx[1].p, c->sum.p);
        // the order by (run, position 0, position 1), the lowest fragment first
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const uint32_t*)c->k32[0].p, c->k32[1].p, (const uint32_t*)c->idx[1].p, c->idx[0].p, (int)nf, 0, 32, st);
        }));
        hipLaunchKernelGGL(k_pos_keys, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const uint32_t*)c->idx[0].p, (const u64*)c->fkey.p, (const int32_t*)c->p0.p, nf,
                           c->k64[0].p);
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
            return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->k64[0].p, c->k64[1].p, (const uint32_t*)c->idx[0].p, c->idx[1].p, (int)nf, 0,
                                                      32 + bits_for(n_runs - 1), st);
        }));
    }
    TASKC_HIP(hipEventRecord(c->ev[6], st));
    if (F) {
        if (const int rc = read_summary(c)) return rc;
        if ((int64_t)sum.miss < nf) {                           // the run's last line, which lies in front of the line stop
            TASKC_HIP(hipMemcpyAsync(&c->h_u64, c->fkey.p + sum.miss, sizeof(u64), hipMemcpyDeviceToHost, st));
            TASKC_HIP(hipStreamSynchronize(st));
            const int64_t run = (int64_t)(c->h_u64 >> 32);
            if (run >= n_runs) return TASKC_FAIL(DSA_E_DEVICE, "internal: run %lld of %lld", (long long)run, (long long)n_runs);
            TASKC_HIP(hipMemcpyAsync(&c->h_u32, c->run_first.p + run + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            TASKC_HIP(hipStreamSynchronize(st));
            const int64_t last = (int64_t)c->h_u32 - 1;
            if (last < 0 || last >= m) return TASKC_FAIL(DSA_E_DEVICE, "internal: run %lld ends at line %lld of %lld", (long long)run, (long long)last, (long long)m);
            return line_stop(c, last, true, TASKC_MISSING_END, (int64_t)(int32_t)((uint32_t)c->h_u64 ^ SIGN), r);
        }
    }
    if (stopped) return line_stop(c, m, true, 0, 0, r);

    // select: duplicates, the kept counts of every run, the output's lines
    for (auto* b : {&c->rlo, &c->rhi}) {
        TASKC_HIP(b->reserve((size_t)n_runs));
        TASKC_HIP(hipMemsetAsync(b->p, 0, (size_t)n_runs * sizeof(uint32_t), st));
    }
    if (nf) {
        TASKC_HIP(c->osrc.reserve(2 * (size_t)nf));
        TASKC_HIP(c->odst.reserve(2 * (size_t)nf));
        hipLaunchKernelGGL(k_dup_heads, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, (const uint32_t*)c->idx[1].p, (const int32_t*)c->p1.p, nf, c->hd.p,
                           c->keepf.p);
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->hd.p, c->hp.p, (int)nf, st); }));
        hipLaunchKernelGGL(k_run_edges, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, (const uint32_t*)c->hd.p, (const uint32_t*)c->hp.p, nf, n_runs,
                           c->rlo.p, c->rhi.p);
    }
    hipLaunchKernelGGL(k_runs_kept, dim3(grid_of(n_runs)), dim3(BLOCK), 0, st, (const uint32_t*)c->rlo.p, (const uint32_t*)c->rhi.p, n_runs, min_size, c->sum.p);
    if (nf) {
        hipLaunchKernelGGL(k_frag_out, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const u64*)c->fkey.p, (const uint32_t*)c->keepf.p, (const uint32_t*)c->rlo.p,
                           (const uint32_t*)c->rhi.p, (const uint32_t*)c->win.p, (const int32_t*)c->llen.p, nf, n_runs, m, min_size, c->of.p, c->flen.p);
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->of.p, c->orank.p, (int)nf, st); }));
        TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->flen.p, c->fdst.p, (int)nf, st); }));
        hipLaunchKernelGGL(k_out_lines, dim3(grid_of(nf)), dim3(BLOCK), 0, st, (const uint32_t*)c->of.p, (const uint32_t*)c->orank.p, (const u64*)c->flen.p,
                           (const u64*)c->fdst.p, (const uint32_t*)c->win.p, (const int32_t*)c->llen.p, nf, c->osrc.p, c->odst.p, c->sum.p);
    }
    TASKC_HIP(hipEventRecord(c->ev[7], st));
    if (const int rc = read_summary(c)) return rc;
    const int64_t kept = (int64_t)sum.n_kept_frags, out_bytes = sum.out_bytes;
    if (kept > nf || out_bytes < 0 || out_bytes > c->n_bytes + n || (int64_t)sum.n_kept_runs > n_runs)
        return TASKC_FAIL(DSA_E_DEVICE, "internal: %lld output bytes of %lld fragments from %lld input bytes", (long long)out_bytes, (long long)kept, (long long)c->n_bytes);

    // gather
    TASKC_HIP(c->dout.reserve((size_t)out_bytes + 8));            // whole dwords
    if (kept)
        hipLaunchKernelGGL(k_gather<LINE_GROUP>, dim3(grid_of(2 * kept * LINE_GROUP)), dim3(BLOCK), 0, st, (const uint32_t*)c->osrc.p, (const u64*)c->odst.p, 2 * kept,
                           (const uint8_t*)c->text.p, c->text_used, (const int64_t*)c->lstart.p, (const int32_t*)c->llen.p, m, c->dout.p, out_bytes);
    TASKC_HIP(hipEventRecord(c->ev[8], st));
    TASKC_HIP(hipStreamSynchronize(st));
    TASKC_HIP(hipGetLastError());
    c->timing.sorts_ms = hiphost::elapsed(c->ev[5], c->ev[6]) - (parsed_before ? 0.f : c->timing.parse_ms);
    c->timing.select_ms = hiphost::elapsed(c->ev[6], c->ev[7]);
    c->timing.gather_ms = hiphost::elapsed(c->ev[7], c->ev[8]);
    c->dout_bytes = out_bytes;
    c->dout_lines = 2 * kept;
    c->has_dedup = true;
    r->n_runs = n_runs;
    r->n_fragments = nf;
    r->n_kept_fragments = kept;
    r->n_kept_runs = (int64_t)sum.n_kept_runs;
    r->out_bytes = out_bytes;
    return DSA_OK;
}

int regions_run(taskc_ctx* c, bool from_dedup, taskc_result* r)
{
    TASKC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    const int64_t q = from_dedup ? c->dout_lines : c->n_lines, m = c->n_lines;
    const uint32_t* src = from_dedup ? c->osrc.p : nullptr;
    r->n_lines = q;
    if (q == 0) {
        c->has_regions = true;
        c->n_groups = from_dedup ? -1 : 0;
        return DSA_OK;
    }
    const bool parsed_before = c->parsed;
    TASKC_HIP(hipEventRecord(c->ev[9], st));
    if (const int rc = ensure_parsed(c)) return rc;
    if (const int rc = reset_summary(c)) return rc;
    Summary& sum = c->h_sum;
    for (auto* b : {&c->k64[0], &c->k64[1], &c->glen, &c->gdst}) TASKC_HIP(b->reserve((size_t)q));
    for (auto* b : {&c->idx[0], &c->idx[1], &c->head, &c->runp, &c->glast}) TASKC_HIP(b->reserve((size_t)q));
    for (auto* b : {&c->vstart, &c->vend, &c->gmin, &c->gmax}) TASKC_HIP(b->reserve((size_t)q));
    TASKC_HIP(c->n_unique.reserve(1));
    hipLaunchKernelGGL(k_region_keys, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const taskc_line*)c->rec.p, src, q, m, c->k64[0].p, c->idx[0].p, c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    if ((int64_t)sum.rstop < q) {
        const int64_t k = sum.rstop;
        int64_t i = k;
        if (from_dedup) {
            TASKC_HIP(hipMemcpyAsync(&c->h_u32, c->osrc.p + k, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            TASKC_HIP(hipMemcpyAsync(&c->h_u64, c->odst.p + k, sizeof(u64), hipMemcpyDeviceToHost, st));
            TASKC_HIP(hipStreamSynchronize(st));
            i = c->h_u32;
            if (i >= m) return TASKC_FAIL(DSA_E_DEVICE, "internal: line %lld of the dedup text is input line %lld of %lld", (long long)k, (long long)i, (long long)m);
        }
        if (const int rc = line_stop(c, i, false, 0, 0, r)) return rc;
        if (from_dedup) {
            r->stop_line = k + 1;
            r->stop_off = (int64_t)c->h_u64;
        }
        return DSA_OK;
    }
    // the order by (id, end); groups; least start, greatest end, last line
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceRadixSort::SortPairs(w, wb, (const u64*)c->k64[0].p, c->k64[1].p, (const uint32_t*)c->idx[0].p, c->idx[1].p, (int)q, 0, 64, st);
    }));
    hipLaunchKernelGGL(k_key_heads, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, q, c->head.p);
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::InclusiveSum(w, wb, c->head.p, c->runp.p, (int)q, st); }));
    hipLaunchKernelGGL(k_region_vals, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)c->k64[1].p, (const uint32_t*)c->idx[1].p, (const uint32_t*)c->runp.p,
                       (const taskc_line*)c->rec.p, src, q, m, c->vstart.p, c->vend.p, c->glast.p, c->sum.p);
    u64* gkey = c->k64[0].p;                                    // (the unsorted keys are done with)
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceReduce::ReduceByKey(w, wb, (const u64*)c->k64[1].p, gkey, (const int32_t*)c->vstart.p, c->gmin.p, c->n_unique.p, hipcub::Min(), (int)q, st);
    }));
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) {
        return hipcub::DeviceReduce::ReduceByKey(w, wb, (const u64*)c->k64[1].p, gkey, (const int32_t*)c->vend.p, c->gmax.p, c->n_unique.p, hipcub::Max(), (int)q, st);
    }));
    hipLaunchKernelGGL(k_region_groups, dim3(grid_of(q)), dim3(BLOCK), 0, st, (const u64*)gkey, (const int32_t*)c->gmin.p, (const int32_t*)c->gmax.p,
                       (const uint32_t*)c->glast.p, (const taskc_line*)c->rec.p, q, m, c->glen.p, c->sum.p);
    TASKC_HIP(hipEventRecord(c->ev[10], st));
    TASKC_HIP(hiphost::cub_run(c->scratch.tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->glen.p, c->gdst.p, (int)q, st); }));
    hipLaunchKernelGGL(k_region_total, dim3(1), dim3(64), 0, st, (const u64*)c->glen.p, (const u64*)c->gdst.p, q, c->sum.p);
    if (const int rc = read_summary(c)) return rc;
    const int64_t n_groups = sum.n_groups, out_bytes = sum.out_bytes;
    if (n_groups < 1 || n_groups > q || (int64_t)sum.n_ids > n_groups || out_bytes < 0)
        return TASKC_FAIL(DSA_E_DEVICE, "internal: %lld groups of %lld lines", (long long)n_groups, (long long)q);
    if ((int64_t)sum.bad_group < n_groups) {
        TASKC_HIP(hipMemcpyAsync(&c->h_u64, gkey + sum.bad_group, sizeof(u64), hipMemcpyDeviceToHost, st));
        TASKC_HIP(hipStreamSynchronize(st));
        r->stop_kind = TASKC_NOT_TWO_ENDS;
        r->stop_value = (int64_t)(int32_t)((uint32_t)(c->h_u64 >> 32) ^ SIGN);
        return DSA_OK;
    }
    TASKC_HIP(c->rout.reserve((size_t)out_bytes + 8));
    hipLaunchKernelGGL(k_region_print<LINE_GROUP>, dim3(grid_of(n_groups * LINE_GROUP)), dim3(BLOCK), 0, st, (const u64*)gkey, (const int32_t*)c->gmin.p,
                       (const int32_t*)c->gmax.p, (const uint32_t*)c->glast.p, (const u64*)c->gdst.p, (const u64*)c->glen.p, (const taskc_line*)c->rec.p,
                       (const uint8_t*)c->text.p, (const int64_t*)c->lstart.p, n_groups, m, c->rout.p, out_bytes);
    TASKC_HIP(hipEventRecord(c->ev[11], st));
    TASKC_HIP(hipStreamSynchronize(st));
    TASKC_HIP(hipGetLastError());
    c->timing.regions_ms = hiphost::elapsed(c->ev[9], c->ev[10]) - (parsed_before ? 0.f : c->timing.parse_ms);
    c->timing.print_ms = hiphost::elapsed(c->ev[10], c->ev[11]);
    c->rout_bytes = out_bytes;
    c->has_regions = true;
    c->n_groups = from_dedup ? -1 : n_groups;
    r->n_clusters = sum.n_ids;
    r->out_bytes = out_bytes;
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* taskc_last_error(void) { return g_taskc_err.c_str(); }

int taskc_create(int device, taskc_ctx** out)
{
    if (!out) return TASKC_FAIL(DSA_E_ARG, "taskc_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_taskc_err)) return DSA_E_DEVICE;
    TASKC_HIP(hipSetDevice(device));
    taskc_ctx* c = new taskc_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete c;
        return TASKC_FAIL(DSA_E_DEVICE, "taskc_create: cannot create a stream or an event");
    }
    *out = c;
    return DSA_OK;
}

void taskc_destroy(taskc_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int taskc_begin(taskc_ctx* c)
{
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_begin: no ctx");
    TASKC_HIP(hipSetDevice(c->device));
    TASKC_HIP(hipStreamSynchronize(c->st));
    c->pieces.clear();
    c->text_used = c->n_lines = c->n_bytes = 0;
    drop_outputs(c);
    c->timing = taskc_timing{};
    return DSA_OK;
}

int taskc_add(taskc_ctx* c, const uint8_t* text, int64_t len, int32_t final, int64_t* consumed)
{
    if (!consumed) return TASKC_FAIL(DSA_E_ARG, "taskc_add: no place for the consumed count");
    *consumed = 0;
    if (len < 0) return TASKC_FAIL(DSA_E_ARG, "taskc_add: negative length (%lld)", (long long)len);
    if (len > (int64_t)INT32_MAX) return TASKC_FAIL(DSA_E_LIMIT, "taskc_add: %lld bytes in one call, more than 2^31 - 1: give the text in pieces", (long long)len);
    if (len && !text) return TASKC_FAIL(DSA_E_ARG, "taskc_add: null pointer with non-zero size");
    if (final != 0 && final != 1) return TASKC_FAIL(DSA_E_ARG, "taskc_add: final %d is not 0 or 1", final);
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_add: no ctx");
    if (!final) len = whole_lines(text, len);
    if (len == 0) return DSA_OK;
    drop_outputs(c);                                            // they are of another input
    const int rc = add_piece(c, text, len, hipMemcpyHostToDevice);
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);        // nothing of a refused call is in flight when it returns
    else *consumed = len;
    return rc;
}

int taskc_add_cover(taskc_ctx* c, const sct_ctx* cover)
{
    if (!c || !cover) return TASKC_FAIL(DSA_E_ARG, "taskc_add_cover: no %s", !c ? "ctx" : "cover");
    int device = -1;
    const uint8_t* text = nullptr;
    int64_t len = 0;
    if (!sct_cover_output_device(cover, &device, &text, &len)) return TASKC_FAIL(DSA_E_ARG, "taskc_add_cover: the cover has no output (sct_cover first)");
    if (device != c->device) return TASKC_FAIL(DSA_E_ARG, "taskc_add_cover: ctx and cover are on devices %d and %d", c->device, device);
    if (len > (int64_t)INT32_MAX) return TASKC_FAIL(DSA_E_LIMIT, "taskc_add_cover: a cover output of %lld bytes, more than 2^31 - 1", (long long)len);
    if (len == 0) return DSA_OK;
    drop_outputs(c);
    const int rc = add_piece(c, text, len, hipMemcpyDeviceToDevice);    // (sct_cover returned: its stream is idle)
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);
    return rc;
}

int taskc_dedup(taskc_ctx* c, int64_t min_cluster_size, taskc_result* r)
{
    if (!r) return TASKC_FAIL(DSA_E_ARG, "taskc_dedup: no result");
    *r = taskc_result{};
    r->stop_field = -1;
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_dedup: no ctx");
    c->has_dedup = c->has_regions = false;                      // (regions of the old dedup text go with it)
    c->dout_bytes = c->dout_lines = c->rout_bytes = 0;
    c->timing.sorts_ms = c->timing.select_ms = c->timing.gather_ms = 0.f;
    if (c->n_lines == 0) {
        c->has_dedup = true;
        return DSA_OK;
    }
    const int rc = dedup_run(c, min_cluster_size, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        *r = taskc_result{};
        r->stop_field = -1;
    } else if (r->stop_kind) (void)hipStreamSynchronize(c->st);
    return rc;
}

int taskc_regions(taskc_ctx* c, int32_t source, taskc_result* r)
{
    if (!r) return TASKC_FAIL(DSA_E_ARG, "taskc_regions: no result");
    *r = taskc_result{};
    r->stop_field = -1;
    if (source != TASKC_INPUT && source != TASKC_DEDUP) return TASKC_FAIL(DSA_E_ARG, "taskc_regions: source %d is neither TASKC_INPUT nor TASKC_DEDUP", source);
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_regions: no ctx");
    c->has_regions = false;
    c->rout_bytes = 0;
    c->timing.regions_ms = c->timing.print_ms = 0.f;
    if (source == TASKC_DEDUP && !c->has_dedup) return TASKC_FAIL(DSA_E_ARG, "taskc_regions: the ctx has no dedup text (taskc_dedup first)");
    const int rc = regions_run(c, source == TASKC_DEDUP, r);
    if (rc != DSA_OK) {
        (void)hipStreamSynchronize(c->st);
        c->has_regions = false;
        *r = taskc_result{};
        r->stop_field = -1;
    } else if (r->stop_kind) (void)hipStreamSynchronize(c->st);
    return rc;
}

int taskc_fetch(taskc_ctx* c, int32_t which, int64_t offset, uint8_t* buf, int64_t len)
{
    if (which != TASKC_DEDUP && which != TASKC_REGIONS) return TASKC_FAIL(DSA_E_ARG, "taskc_fetch: which %d is neither TASKC_DEDUP nor TASKC_REGIONS", which);
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_fetch: no ctx");
    const bool dedup = which == TASKC_DEDUP;
    if (!(dedup ? c->has_dedup : c->has_regions)) return TASKC_FAIL(DSA_E_ARG, "taskc_fetch: the ctx has no %s text", dedup ? "dedup" : "regions");
    const int64_t bytes = dedup ? c->dout_bytes : c->rout_bytes;
    if (offset < 0 || len < 0 || offset > bytes || len > bytes - offset)
        return TASKC_FAIL(DSA_E_ARG, "taskc_fetch: [%lld, +%lld) is outside the %lld bytes", (long long)offset, (long long)len, (long long)bytes);
    if (len && !buf) return TASKC_FAIL(DSA_E_ARG, "taskc_fetch: length without a buffer");
    if (len == 0) return DSA_OK;
    TASKC_HIP(hipSetDevice(c->device));
    TASKC_HIP(hipMemcpyAsync(buf, (dedup ? c->dout.p : c->rout.p) + offset, (size_t)len, hipMemcpyDeviceToHost, c->st));
    TASKC_HIP(hipStreamSynchronize(c->st));
    return DSA_OK;
}

int taskc_parse_regions(taskc_ctx* c, taskt_ctx* into, const taskt_names* seq_names, taskt_result* result)
{
    if (!c) return TASKC_FAIL(DSA_E_ARG, "taskc_parse_regions: no ctx");
    if (!c->has_regions) return TASKC_FAIL(DSA_E_ARG, "taskc_parse_regions: the ctx has no regions text (taskc_regions first)");
    const int rc = taskt_regions_from_device(into, seq_names, c->device, c->rout.p, c->rout_bytes, result);
    if (rc != DSA_OK) return TASKC_FAIL(rc, "taskc_parse_regions: %s", taskt_last_error());
    return DSA_OK;
}

int taskc_get_timing(const taskc_ctx* c, taskc_timing* out)
{
    if (!c || !out) return TASKC_FAIL(DSA_E_ARG, "taskc_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"

// For span_api.hip: the parsed lines of the input (from_dedup false) or of the dedup text, where they lie.  Parses the input if
// no step has yet; the ctx's stream is idle on return.  DSA_E_ARG (its text in taskc_last_error()) without a dedup text.
__attribute__((visibility("hidden"))) int taskc_lines_device(taskc_ctx* c, bool from_dedup, taskc_lines_view* out)
{
    if (from_dedup && !c->has_dedup) return TASKC_FAIL(DSA_E_ARG, "the ctx has no dedup text (taskc_dedup first)");
    TASKC_HIP(hipSetDevice(c->device));
    if (const int rc = ensure_parsed(c)) {
        (void)hipStreamSynchronize(c->st);
        return rc;
    }
    *out = taskc_lines_view{c->device, c->text.p, c->lstart.p, c->llen.p, c->rec.p, from_dedup ? c->osrc.p : nullptr, c->n_lines,
                            from_dedup ? c->dout_lines : c->n_lines};
    return DSA_OK;
}

// For conc_api.hip: the groups by (id, end) that taskc_regions(TASKC_INPUT) last made, in key order: the key (id, end, either with
// the sign bit turned), the least start, the greatest end and the input line that is the group's last.  Device pointers, valid
// until the next call on the taskc_ctx.  DSA_E_ARG unless the regions text is the input's.
__attribute__((visibility("hidden"))) int taskc_groups_device(taskc_ctx* c, taskc_groups_view* out)
{
    if (!c->has_regions || c->n_groups < 0) return TASKC_FAIL(DSA_E_ARG, "the ctx has no regions text of its input (taskc_regions(TASKC_INPUT) first)");
    *out = taskc_groups_view{c->k64[0].p, c->gmin.p, c->gmax.p, c->glast.p, c->n_groups};
    return DSA_OK;
}

// For conc_api.hip (conc_into_taskc): a piece from this device's memory, as taskc_add_cover adds one.
__attribute__((visibility("hidden"))) int taskc_add_device(taskc_ctx* c, int device, const uint8_t* text, int64_t len)
{
    if (device != c->device) return TASKC_FAIL(DSA_E_ARG, "the ctx and the text are on devices %d and %d", c->device, device);
    if (len > (int64_t)INT32_MAX) return TASKC_FAIL(DSA_E_LIMIT, "a text of %lld bytes, more than 2^31 - 1", (long long)len);
    if (len == 0) return DSA_OK;
    drop_outputs(c);
    const int rc = add_piece(c, text, len, hipMemcpyDeviceToDevice);
    if (rc != DSA_OK) (void)hipStreamSynchronize(c->st);
    return rc;
}
