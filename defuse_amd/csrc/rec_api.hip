// rec_api.hip — the record store of include/defuse_rec.h on gfx950: the split-alignment records of many batches in one
// device array, sorted into the order of the pipeline's `LC_ALL=C sort -n -k 1` on their lines, and those lines printed.
//
// Sort, n records (rec_shared.hpp has the keys):
//   k_rec_keys      one thread per record: the 40 bytes as dwordx4 + dwordx4 + dwordx2 -> nine key columns (the biased fusion
//                   id and the 44-bit keys of fields 2-9), the identity permutation, and a flag if a read_end or revcomp is
//                   not 0 or 1
//   stable radix sorts of (64-bit key, 32-bit index), least significant field first, each over the bits its key has: score,
//                   read_second, read_first, ref_second, ref_first (44 bits), then frag with read_end and revcomp as two
//                   bits beside it (46 bits) — or, with the flag up, revcomp, read_end and frag by their full keys — and
//                   the fusion id last (32 bits).  Between two sorts k_rec_pass_key / k_rec_cand_key fetch the next column
//                   in the current order.
//   k_rec_permute   the records in the final order into the second record buffer: one thread per 8 bytes of OUTPUT, so the
//                   writes are coalesced and the reads are 40-byte runs; the two buffers then change places.
// Text, m lines (all records, or a kept list copied to the device):
//   k_rec_len       the length of each line; a 64-bit ExclusiveSum gives each line's offset and the size of the text
//   k_rec_write     a workgroup's 256 consecutive lines are one contiguous span of the text (at most 256 * 109 bytes): it is
//                   composed in LDS at the span's own alignment modulo 16 and leaves as aligned 16-byte stores, all lanes
//                   to consecutive addresses; the bytes before the first and after the last aligned address go out one by one.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <string>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_rec.h"
#include "hip_host.hpp"
#include "rec_shared.hpp"

namespace {

using hiphost::DeviceBuffer;
using hiphost::grid_of;
using hiphost::GrowSize;

thread_local std::string g_rec_err;

#define REC_HIP(call) HIPHOST_TRY(g_rec_err, call)

constexpr int BLOCK = 256;
constexpr int N_KEYS = REC_FIELDS;                   // key columns: 0 the fusion id, k the field printed (k + 1)th
constexpr int K_FUSION = 0, K_FRAG = 1, K_READ_END = 2, K_REVCOMP = 3, K_SCORE = 8;
constexpr int FUSION_BITS = 32, CAND_BITS = REC_FIELD_KEY_BITS + 2;
constexpr int SPAN_BYTES = BLOCK * REC_MAX_LINE + 16;                 // a workgroup's lines and the span's offset in its first 16 bytes

static_assert(sizeof(dsa_record) == 40 && sizeof(rec_timing) == 56, "C ABI layout");
static_assert(SPAN_BYTES % 16 == 0 && SPAN_BYTES <= 64 * 1024, "LDS span");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// A record is ten ints at a multiple of 40 bytes from an allocation's start: 8-byte aligned, which is all a global load asks for.
__device__ inline dsa_record rec_load(const dsa_record* p)
{
    const char* b = static_cast<const char*>(__builtin_assume_aligned(p, 8));
    u32x4 lo, mid;
    u32x2 hi;
    __builtin_memcpy(&lo, b, 16);
    __builtin_memcpy(&mid, b + 16, 16);
    __builtin_memcpy(&hi, b + 32, 8);
    dsa_record r;
    r.fusion_id = (int32_t)lo.x; r.frag = (int32_t)lo.y; r.read_end = (int32_t)lo.z; r.revcomp = (int32_t)lo.w;
    r.ref_first = (int32_t)mid.x; r.ref_second = (int32_t)mid.y; r.read_first = (int32_t)mid.z; r.read_second = (int32_t)mid.w;
    r.score = (int32_t)hi.x; r.pair_idx = (int32_t)hi.y;
    return r;
}

// keys: N_KEYS columns of `stride` entries
__global__ void __launch_bounds__(BLOCK) k_rec_keys(const dsa_record* __restrict__ rec, int64_t n, uint64_t* __restrict__ keys, int64_t stride,
                                                    uint32_t* __restrict__ idx, uint32_t* __restrict__ wide)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const dsa_record r = rec_load(rec + i);
    const int32_t* f = rec_fields(r);
    keys[i] = rec_fusion_key(r.fusion_id);
#pragma unroll
    for (int k = 1; k < N_KEYS; ++k) keys[k * stride + i] = rec_field_key(f[k]);
    idx[i] = (uint32_t)i;
    if (((uint32_t)r.read_end | (uint32_t)r.revcomp) > 1u) *wide = 1u;          // (every writer stores the same word)
}

// one key column in the current order
__global__ void k_rec_pass_key(const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx, int64_t n, uint64_t* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    out[j] = key[idx[j]];
}

// the candidate's key where every read_end and revcomp is 0 or 1: they are the two low bits under the frag key
__global__ void k_rec_cand_key(const uint64_t* __restrict__ frag, const uint64_t* __restrict__ read_end, const uint64_t* __restrict__ revcomp,
                               const uint32_t* __restrict__ idx, int64_t n, uint64_t* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx[j];
    out[j] = (frag[i] << 2) | (read_end[i] != REC_KEY_OF_0 ? 2u : 0u) | (revcomp[i] != REC_KEY_OF_0 ? 1u : 0u);
}

// a record is five 8-byte words; n_words = 5 n
__global__ void k_rec_permute(const u32x2* __restrict__ in, const uint32_t* __restrict__ idx, int64_t n_words, u32x2* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_words) return;
    const int64_t j = t / 5;
    out[t] = in[(int64_t)idx[j] * 5 + (t - j * 5)];
}

// len[0 .. m] with len[m] = 0, so that the exclusive sum's last entry is the size of the text
__global__ void k_rec_len(const dsa_record* __restrict__ rec, const int64_t* __restrict__ kept, int64_t m, uint64_t* __restrict__ len)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j > m) return;
    uint64_t l = 0;
    if (j < m) l = (uint64_t)rec_line_length(rec_load(rec + (kept ? kept[j] : j)));
    len[j] = l;
}

// file comment.  off[0 .. m]: the text offsets of the lines and the text's size.  LDS byte k holds text byte base + k, base being
// the span's begin rounded down to 16, so that an aligned 16-byte read of LDS is an aligned 16-byte store of the text.
__global__ void __launch_bounds__(BLOCK) k_rec_write(const dsa_record* __restrict__ rec, const int64_t* __restrict__ kept, int64_t m,
                                                     const uint64_t* __restrict__ off, char* __restrict__ text)
{
    __shared__ __attribute__((aligned(16))) char span[SPAN_BYTES];
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int64_t last = first + BLOCK < m ? first + BLOCK : m;
    const uint64_t begin = off[first], end = off[last];
    const uint64_t base = begin & ~(uint64_t)15;
    const int64_t j = first + threadIdx.x;
    if (j < m) rec_write_line(rec_load(rec + (kept ? kept[j] : j)), span + (off[j] - base));
    __syncthreads();
    const uint64_t up = (begin + 15) & ~(uint64_t)15, down = end & ~(uint64_t)15;
    const uint64_t head_end = up < end ? up : end;                  // [begin, head_end): before the first aligned address
    const uint64_t tail_begin = down > head_end ? down : head_end;  // [tail_begin, end): after the last one
    for (uint64_t a = head_end + (uint64_t)threadIdx.x * 16; a < tail_begin; a += (uint64_t)BLOCK * 16)
        *reinterpret_cast<u32x4*>(text + a) = *reinterpret_cast<const u32x4*>(span + (a - base));
    if (threadIdx.x < 16) {
        const uint64_t a = begin + threadIdx.x;
        if (a < head_end) text[a] = span[a - base];
    } else if (threadIdx.x >= 64 && threadIdx.x < 80) {             // another wavefront
        const uint64_t a = tail_begin + (threadIdx.x - 64);
        if (a < end) text[a] = span[a - base];
    }
}

enum { EV_A0, EV_A1, EV_K0, EV_K1, EV_S1, EV_G1, EV_F0, EV_F1, EV_F2, EV_F3, EV_D0, EV_D1, N_EVENTS };

}  // namespace

struct rec_store {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[N_EVENTS];
    rec_timing timing{};
    int64_t n = 0;
    int64_t tail_room = -1;                                         // of the rec_tail that awaits its rec_commit; -1: none
    DeviceBuffer<dsa_record, GrowSize> rec, rec_alt;                // the records, and where the next sort writes them
    DeviceBuffer<uint64_t, GrowSize> keys, key_in, key_out, len, off;
    DeviceBuffer<uint32_t, GrowSize> idx_a, idx_b;
    DeviceBuffer<uint32_t> wide;
    DeviceBuffer<int64_t, GrowSize> kept;
    DeviceBuffer<char, GrowSize> text;
    DeviceBuffer<uint8_t, GrowSize> tmp;
};

namespace {

// 32-bit indices and sort counts; the bound eval_groups has
int rec_check_total(const rec_store* s, int64_t more, const char* who)
{
    if (more >= INT32_MAX - 1 || s->n + more >= INT32_MAX - 1)
        return hiphost::fail(g_rec_err, DSA_E_LIMIT, "%s: a store holds fewer than 2^31 - 2 records", who);
    return DSA_OK;
}

// room for `need` records; what the store holds moves to the new buffer device to device (on the stream, not waited for)
int rec_make_room(rec_store* s, int64_t need)
{
    if (s->rec.p && (size_t)need <= s->rec.cap) return DSA_OK;
    DeviceBuffer<dsa_record, GrowSize> grown;
    REC_HIP(grown.reserve((size_t)need));
    if (s->n) {
        REC_HIP(hipMemcpyAsync(grown.p, s->rec.p, (size_t)s->n * sizeof(dsa_record), hipMemcpyDeviceToDevice, s->st));
        REC_HIP(hipStreamSynchronize(s->st));                       // before the old buffer is freed
    }
    s->rec.swap(grown);
    return DSA_OK;
}

int rec_append_any(rec_store* s, const void* records, int64_t n, bool on_device, const char* who)
{
    if (!s || n < 0 || (n && !records)) return hiphost::fail(g_rec_err, DSA_E_ARG, "%s: null pointer or negative count", who);
    if (const int rc = rec_check_total(s, n, who)) return rc;
    s->tail_room = -1;
    if (n == 0) return DSA_OK;
    REC_HIP(hipSetDevice(s->device));
    REC_HIP(hipEventRecord(s->ev[EV_A0], s->st));
    if (const int rc = rec_make_room(s, s->n + n)) return rc;
    REC_HIP(hipMemcpyAsync(s->rec.p + s->n, records, (size_t)n * sizeof(dsa_record), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
    REC_HIP(hipEventRecord(s->ev[EV_A1], s->st));
    REC_HIP(hipStreamSynchronize(s->st));
    s->timing.append_ms += hiphost::elapsed(s->ev[EV_A0], s->ev[EV_A1]);
    s->n += n;
    s->timing.n_records = s->n;
    return DSA_OK;
}

// one stable sort of (key, index) over key bits [0, bits); cur and next change places
int rec_sort_pass(rec_store* s, const uint64_t* key, int bits, uint32_t*& cur, uint32_t*& next)
{
    const int n = (int)s->n;
    hipStream_t st = s->st;
    uint64_t* sorted = s->key_out.p;
    const uint32_t* in = cur;
    uint32_t* out = next;
    REC_HIP(hiphost::cub_run(s->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceRadixSort::SortPairs(t, tb, key, sorted, in, out, n, 0, bits, st);
    }));
    std::swap(cur, next);
    ++s->timing.n_sorts;
    return DSA_OK;
}

}  // namespace

// for rect_api.hip, which must refuse a store of another device before it touches either (not part of the C ABI)
__attribute__((visibility("hidden"))) int recstore_device(const rec_store* s) { return s->device; }

extern "C" {

const char* rec_last_error(void) { return g_rec_err.c_str(); }

int rec_create(int device, rec_store** out)
{
    if (!out) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_create: null pointer");
    *out = nullptr;
    if (hiphost::check_device(device, &g_rec_err)) return DSA_E_DEVICE;
    REC_HIP(hipSetDevice(device));
    rec_store* s = new rec_store();
    s->device = device;
    bool ok = s->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : s->ev) ok = ok && e.create() == hipSuccess;
    if (!ok) {
        delete s;
        return hiphost::fail(g_rec_err, DSA_E_DEVICE, "rec_create: cannot create a stream");
    }
    *out = s;
    return DSA_OK;
}

void rec_destroy(rec_store* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    delete s;
}

int rec_clear(rec_store* s)
{
    if (!s) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_clear: null pointer");
    s->n = 0;
    s->tail_room = -1;
    s->timing = rec_timing{};
    return DSA_OK;
}

int rec_append(rec_store* s, const dsa_record* records, int64_t n) { return rec_append_any(s, records, n, false, "rec_append"); }

int rec_append_device(rec_store* s, const void* records_device, int64_t n) { return rec_append_any(s, records_device, n, true, "rec_append_device"); }

int rec_tail(rec_store* s, int64_t room, void** tail_device)
{
    if (!s || room < 0 || !tail_device) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_tail: null pointer or negative room");
    *tail_device = nullptr;
    if (const int rc = rec_check_total(s, room, "rec_tail")) return rc;
    s->tail_room = -1;
    REC_HIP(hipSetDevice(s->device));
    REC_HIP(hipEventRecord(s->ev[EV_A0], s->st));
    if (const int rc = rec_make_room(s, s->n + room)) return rc;
    REC_HIP(hipEventRecord(s->ev[EV_A1], s->st));
    REC_HIP(hipStreamSynchronize(s->st));
    s->timing.append_ms += hiphost::elapsed(s->ev[EV_A0], s->ev[EV_A1]);
    *tail_device = s->rec.p + s->n;
    s->tail_room = room;
    return DSA_OK;
}

int rec_commit(rec_store* s, int64_t n)
{
    if (!s || n < 0) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_commit: null pointer or negative count");
    if (s->tail_room < 0) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_commit: no rec_tail awaits a commit");
    if (n > s->tail_room) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_commit: %lld records, but rec_tail gave room for %lld", (long long)n, (long long)s->tail_room);
    s->n += n;
    s->tail_room = -1;
    s->timing.n_records = s->n;
    return DSA_OK;
}

int rec_sort(rec_store* s)
{
    if (!s) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_sort: null pointer");
    s->tail_room = -1;
    s->timing.keys_ms = s->timing.sort_ms = s->timing.gather_ms = 0.f;
    s->timing.n_sorts = 0;
    const int64_t n = s->n;
    if (n <= 1) return DSA_OK;
    REC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->st;
    REC_HIP(s->keys.reserve((size_t)n * N_KEYS));
    REC_HIP(s->key_in.reserve((size_t)n));
    REC_HIP(s->key_out.reserve((size_t)n));
    REC_HIP(s->idx_a.reserve((size_t)n));
    REC_HIP(s->idx_b.reserve((size_t)n));
    REC_HIP(s->rec_alt.reserve((size_t)n));
    REC_HIP(s->wide.reserve(1));
    const unsigned g = grid_of(n);
    uint64_t* K = s->keys.p;
    const auto column = [&](int k) { return K + (int64_t)k * n; };
    uint32_t wide = 0;
    REC_HIP(hipEventRecord(s->ev[EV_K0], st));
    REC_HIP(hipMemsetAsync(s->wide.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_rec_keys, dim3(g), dim3(BLOCK), 0, st, s->rec.p, n, K, n, s->idx_a.p, s->wide.p);
    REC_HIP(hipEventRecord(s->ev[EV_K1], st));
    REC_HIP(hipMemcpyAsync(&wide, s->wide.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    REC_HIP(hipStreamSynchronize(st));                              // the schedule depends on the flag
    REC_HIP(hipGetLastError());
    uint32_t *cur = s->idx_a.p, *next = s->idx_b.p;
    // least significant first; the first sort reads its column in place (the permutation is still the identity)
    if (const int rc = rec_sort_pass(s, column(K_SCORE), REC_FIELD_KEY_BITS, cur, next)) return rc;
    for (int k = K_SCORE - 1; k > (wide ? K_FUSION : K_REVCOMP); --k) {
        hipLaunchKernelGGL(k_rec_pass_key, dim3(g), dim3(BLOCK), 0, st, column(k), cur, n, s->key_in.p);
        if (const int rc = rec_sort_pass(s, s->key_in.p, REC_FIELD_KEY_BITS, cur, next)) return rc;
    }
    if (!wide) {
        hipLaunchKernelGGL(k_rec_cand_key, dim3(g), dim3(BLOCK), 0, st, column(K_FRAG), column(K_READ_END), column(K_REVCOMP), cur, n, s->key_in.p);
        if (const int rc = rec_sort_pass(s, s->key_in.p, CAND_BITS, cur, next)) return rc;
    }
    hipLaunchKernelGGL(k_rec_pass_key, dim3(g), dim3(BLOCK), 0, st, column(K_FUSION), cur, n, s->key_in.p);
    if (const int rc = rec_sort_pass(s, s->key_in.p, FUSION_BITS, cur, next)) return rc;
    REC_HIP(hipEventRecord(s->ev[EV_S1], st));
    hipLaunchKernelGGL(k_rec_permute, dim3(grid_of(n * 5)), dim3(BLOCK), 0, st, reinterpret_cast<const u32x2*>(s->rec.p), cur, n * 5,
                       reinterpret_cast<u32x2*>(s->rec_alt.p));
    REC_HIP(hipEventRecord(s->ev[EV_G1], st));
    REC_HIP(hipStreamSynchronize(st));
    REC_HIP(hipGetLastError());
    s->rec.swap(s->rec_alt);
    s->timing.keys_ms = hiphost::elapsed(s->ev[EV_K0], s->ev[EV_K1]);
    s->timing.sort_ms = hiphost::elapsed(s->ev[EV_K1], s->ev[EV_S1]);
    s->timing.gather_ms = hiphost::elapsed(s->ev[EV_S1], s->ev[EV_G1]);
    return DSA_OK;
}

int rec_count(const rec_store* s, int64_t* n)
{
    if (!s || !n) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_count: null pointer");
    *n = s->n;
    return DSA_OK;
}

int rec_records_device(const rec_store* s, const void** records_device, int64_t* n)
{
    if (!s || !records_device || !n) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_records_device: null pointer");
    *records_device = s->rec.p;
    *n = s->n;
    return DSA_OK;
}

int rec_download(rec_store* s, dsa_record* out, int64_t cap, int64_t* n)
{
    if (!s || !n || cap < 0) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_download: null pointer or negative capacity");
    *n = s->n;
    s->timing.download_ms = 0.f;
    if (s->n > cap) return hiphost::fail(g_rec_err, DSA_E_CAPACITY, "rec_download: %lld records do not fit %lld", (long long)s->n, (long long)cap);
    if (s->n == 0) return DSA_OK;
    if (!out) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_download: null output pointer");
    REC_HIP(hipSetDevice(s->device));
    REC_HIP(hipEventRecord(s->ev[EV_D0], s->st));
    REC_HIP(hipMemcpyAsync(out, s->rec.p, (size_t)s->n * sizeof(dsa_record), hipMemcpyDeviceToHost, s->st));
    REC_HIP(hipEventRecord(s->ev[EV_D1], s->st));
    REC_HIP(hipStreamSynchronize(s->st));
    s->timing.download_ms = hiphost::elapsed(s->ev[EV_D0], s->ev[EV_D1]);
    return DSA_OK;
}

int rec_text(rec_store* s, const int64_t* kept, int64_t n_kept, char* out, int64_t cap, int64_t* bytes)
{
    if (!s || !bytes || cap < 0 || (kept && n_kept < 0)) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_text: null pointer or negative count");
    *bytes = 0;
    s->timing.format_ms = s->timing.write_ms = s->timing.download_ms = 0.f;
    s->timing.text_bytes = 0;
    const int64_t m = kept ? n_kept : s->n;
    for (int64_t k = 0; kept && k < m; ++k)
        if (kept[k] < 0 || kept[k] >= s->n)
            return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_text: kept[%lld] = %lld is outside the store's %lld records", (long long)k, (long long)kept[k], (long long)s->n);
    if (m == 0) return DSA_OK;
    if (m >= INT32_MAX - 1) return hiphost::fail(g_rec_err, DSA_E_LIMIT, "rec_text: fewer than 2^31 - 2 lines in one call");
    REC_HIP(hipSetDevice(s->device));
    hipStream_t st = s->st;
    REC_HIP(s->len.reserve((size_t)m + 1));
    REC_HIP(s->off.reserve((size_t)m + 1));
    const int64_t* kept_device = nullptr;
    if (kept) {
        REC_HIP(s->kept.reserve((size_t)m));
        REC_HIP(hipMemcpyAsync(s->kept.p, kept, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st));
        kept_device = s->kept.p;
    }
    REC_HIP(hipEventRecord(s->ev[EV_F0], st));
    hipLaunchKernelGGL(k_rec_len, dim3(grid_of(m + 1)), dim3(BLOCK), 0, st, s->rec.p, kept_device, m, s->len.p);
    uint64_t *len = s->len.p, *off = s->off.p;                      // 64-bit in, 64-bit out: the sum is formed in 64 bits
    REC_HIP(hiphost::cub_run(s->tmp, [&](void* t, size_t& tb) {
        return hipcub::DeviceScan::ExclusiveSum(t, tb, len, off, (int)(m + 1), st);
    }));
    REC_HIP(hipEventRecord(s->ev[EV_F1], st));
    uint64_t total = 0;
    REC_HIP(hipMemcpyAsync(&total, off + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    REC_HIP(hipStreamSynchronize(st));
    REC_HIP(hipGetLastError());
    if (total < (uint64_t)m * (2 * REC_FIELDS + 1) || total > (uint64_t)m * REC_MAX_LINE) return hiphost::fail(g_rec_err, DSA_E_DEVICE, "rec_text: internal: text size out of range");
    *bytes = (int64_t)total;
    s->timing.text_bytes = (int64_t)total;
    if ((int64_t)total > cap) return hiphost::fail(g_rec_err, DSA_E_CAPACITY, "rec_text: %lld bytes do not fit %lld", (long long)total, (long long)cap);
    if (!out) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_text: null output pointer");
    REC_HIP(s->text.reserve((size_t)total));
    REC_HIP(hipEventRecord(s->ev[EV_F2], st));
    hipLaunchKernelGGL(k_rec_write, dim3(grid_of(m)), dim3(BLOCK), 0, st, s->rec.p, kept_device, m, off, s->text.p);
    REC_HIP(hipEventRecord(s->ev[EV_F3], st));
    REC_HIP(hipEventRecord(s->ev[EV_D0], st));
    REC_HIP(hipMemcpyAsync(out, s->text.p, (size_t)total, hipMemcpyDeviceToHost, st));
    REC_HIP(hipEventRecord(s->ev[EV_D1], st));
    REC_HIP(hipStreamSynchronize(st));
    REC_HIP(hipGetLastError());
    s->timing.write_ms = hiphost::elapsed(s->ev[EV_F2], s->ev[EV_F3]);
    s->timing.format_ms = hiphost::elapsed(s->ev[EV_F0], s->ev[EV_F1]) + s->timing.write_ms;
    s->timing.download_ms = hiphost::elapsed(s->ev[EV_D0], s->ev[EV_D1]);
    return DSA_OK;
}

int rec_get_timing(const rec_store* s, rec_timing* out)
{
    if (!s || !out) return hiphost::fail(g_rec_err, DSA_E_ARG, "rec_get_timing: null pointer");
    *out = s->timing;
    out->n_records = s->n;
    return DSA_OK;
}

}  // extern "C"
