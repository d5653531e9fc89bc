// pred_api.hip — the rest of SplitAlignmentTask::Evaluate (tools/SplitAlignment.cpp:545-569, 589-591) for all groups of a
// batch on gfx950 (include/defuse_pred.h): per group the predicted sequence, the two break positions and the two averages,
// from the groups of eval_groups* and the windows that bat_windows_create left on the device.
//
// Tasks (pred_tasks_create).  The host looks at every task anyway to refuse a double fusion_id, so the tasks go up sorted by
// fusion_id (as unsigned, the order of bat_windows), each with the offsets of its two windows in the windows' byte pool: the
// kernels never search the window store.  The remainder sequences are the only bytes copied.
//
// Prediction (pred_predict*), all on the ctx's stream, one host round trip:
//   (1) plan: one thread per group finds its task by binary search, runs the checks of the header and writes the group's
//       row but for seq_off, and its length;
//   (2) a 64-bit exclusive sum of the lengths gives seq_off; the total comes back in one small copy and sizes seq_bytes;
//   (3) descriptors: one thread per group writes seq_off, the '|' byte and four copy segments, two into the remainder bytes
//       and two into the windows' pool (zero-length ones for a group without a sequence);
//   (4) the gather (k_bat_gather of bat_shared.hpp, without its reverse/complement branch and with 64-bit output offsets)
//       copies the segments: the remainders, then the window parts.
// Every byte of seq_bytes has one writer: a segment's group, or the descriptor thread for the separator.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <string>
#include <vector>

#include "../../include/defuse_pred.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"
#include "pred_shared.hpp"

namespace {

using batdev::Seg64;
using predint::DevTask;
using batdev::SRC_PAD;
using hiphost::DeviceBuffer;
using hiphost::GrowSize;
using hiphost::grid_of;
using u64 = unsigned long long;

thread_local std::string g_pred_err;

#define PRED_HIP(call) HIPHOST_TRY(g_pred_err, call)
#define PRED_FAIL(code, ...) hiphost::fail(g_pred_err, code, __VA_ARGS__)

constexpr int BLOCK = batdev::GATHER_BLOCK;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int REM_GROUP = 16;         // lanes per remainder: none to a few hundred bases
constexpr int WINDOW_GROUP = 64;      // lanes per window part: a few hundred bases and more

static_assert(sizeof(pred_task) == 56 && sizeof(pred_result) == 56 && sizeof(pred_device_view) == 40 && sizeof(pred_timing) == 40, "C ABI layout");

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

// tidx[g]: the task of a group that gets a sequence, NONE for every other group
__global__ __launch_bounds__(BLOCK) void k_pred_plan(const eval_group* __restrict__ groups, int64_t n, const uint32_t* __restrict__ tkey,
                                                      const DevTask* __restrict__ task, int64_t n_tasks, pred_result* __restrict__ res,
                                                      u64* __restrict__ len, uint32_t* __restrict__ tidx)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const eval_group e = groups[g];
    pred_result r{};
    r.fusion_id = e.fusion_id;
    r.status = e.status;
    r.count = e.count;
    const int64_t p = lower_bound(tkey, n_tasks, (uint32_t)e.fusion_id);
    uint32_t ti = NONE;
    u64 total = 0;
    if (!(p < n_tasks && tkey[p] == (uint32_t)e.fusion_id)) {
        r.status |= PRED_NO_TASK;
    } else if (!(e.status & EVAL_NO_SPLIT)) {
        const DevTask t = task[p];
        const int64_t first = e.best_first, cut = (int64_t)e.best_second + 1;          // seq0[0 : first), seq1[cut : )
        const int64_t w0 = t.seq_len[0] > 0 ? t.seq_len[0] : 0, w1 = t.seq_len[1] > 0 ? t.seq_len[1] : 0;      // the windows' lengths
        if (first < 0 || first > w0 || cut < 0 || cut >= w1) {
            r.status |= PRED_OUT_OF_WINDOW;
        } else {
            ti = (uint32_t)p;
            total = (u64)t.rem_len[0] + (u64)first + 1u + (u64)(w1 - cut) + (u64)t.rem_len[1];
            r.seq_len = (int32_t)total;                                                 // (pred_tasks_create has bounded it)
            r.break_pos[0] = (int32_t)(t.seq_strand[0] == 0 ? t.seq_start[0] + first - 1 : (int64_t)t.seq_start[0] + t.seq_len[0] - first);
            r.break_pos[1] = (int32_t)(t.seq_strand[1] == 0 ? t.seq_start[1] + cut : (int64_t)t.seq_start[1] + t.seq_len[1] - cut - 1);
            if (!(e.status & EVAL_HOST_STATS)) {
                r.pos_avg = e.pos_sum / (double)e.count;
                r.min_avg = e.min_sum / (double)e.count;
            }
        }
    }
    res[g] = r;
    len[g] = total;
    tidx[g] = ti;
}

__global__ __launch_bounds__(BLOCK) void k_pred_segments(const eval_group* __restrict__ groups, int64_t n, const DevTask* __restrict__ task, int64_t n_tasks,
                                                          const uint32_t* __restrict__ tidx, const u64* __restrict__ off, pred_result* __restrict__ res,
                                                          Seg64* __restrict__ seg_rem, Seg64* __restrict__ seg_win, uint8_t* __restrict__ out, int64_t out_len)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n) return;
    const int64_t o = (int64_t)off[g];
    res[g].seq_off = o;
    Seg64 r0{0, 0, 0, 0}, r1 = r0, w0 = r0, w1 = r0;
    const uint32_t ti = tidx[g];
    if ((int64_t)ti < n_tasks) {
        const DevTask t = task[ti];
        const int64_t first = groups[g].best_first, cut = (int64_t)groups[g].best_second + 1;
        const int64_t bar = o + t.rem_len[0] + first, tail = (int64_t)t.seq_len[1] - cut;         // (seq_len[1] > cut >= 0 here)
        r0 = Seg64{t.rem_off[0], o, (uint32_t)t.rem_len[0], 0};
        w0 = Seg64{(int64_t)t.win_off[0], o + t.rem_len[0], (uint32_t)first, 0};
        if (bar >= 0 && bar < out_len) out[bar] = (uint8_t)'|';
        w1 = Seg64{(int64_t)t.win_off[1] + cut, bar + 1, (uint32_t)tail, 0};
        r1 = Seg64{t.rem_off[1], bar + 1 + tail, (uint32_t)t.rem_len[1], 0};
    }
    seg_rem[2 * g] = r0;
    seg_rem[2 * g + 1] = r1;
    seg_win[2 * g] = w0;
    seg_win[2 * g + 1] = w1;
}

}  // namespace

namespace {

// everything after the groups are on the device (c->ev[1] recorded)
int predict_on_device(pred_ctx* c, const pred_tasks* t, const eval_group* groups, int64_t n)
{
    hipStream_t st = c->st;
    const unsigned gn = grid_of(n);
    PRED_HIP(c->results.reserve((size_t)n));
    PRED_HIP(c->len.reserve((size_t)n));
    PRED_HIP(c->off.reserve((size_t)n));
    PRED_HIP(c->tidx.reserve((size_t)n));
    PRED_HIP(c->seg_rem.reserve((size_t)(2 * n)));
    PRED_HIP(c->seg_win.reserve((size_t)(2 * n)));
    // (1) plan
    hipLaunchKernelGGL(k_pred_plan, dim3(gn), dim3(BLOCK), 0, st, groups, n, (const uint32_t*)t->tkey.p, (const DevTask*)t->task.p, t->n, c->results.p,
                       c->len.p, c->tidx.p);
    PRED_HIP(hipEventRecord(c->ev[2], st));
    // (2) offsets and the total, in 64 bits
    PRED_HIP(hiphost::cub_run(c->tmp, [&](void* w, size_t& wb) { return hipcub::DeviceScan::ExclusiveSum(w, wb, c->len.p, c->off.p, (int)n, st); }));
    u64 last[2] = {0, 0};
    PRED_HIP(hipMemcpyAsync(&last[0], c->off.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    PRED_HIP(hipMemcpyAsync(&last[1], c->len.p + (n - 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    PRED_HIP(hipStreamSynchronize(st));
    PRED_HIP(hipGetLastError());
    const u64 total = last[0] + last[1];
    if (total > (u64)n * (u64)INT32_MAX) return PRED_FAIL(DSA_E_DEVICE, "internal: %llu sequence bytes of %lld groups", total, (long long)n);
    const int64_t SB = (int64_t)total;
    PRED_HIP(c->seq_bytes.reserve((size_t)SB + 4));           // whole dwords
    // (3) descriptors
    hipLaunchKernelGGL(k_pred_segments, dim3(gn), dim3(BLOCK), 0, st, groups, n, (const DevTask*)t->task.p, t->n, (const uint32_t*)c->tidx.p,
                       (const u64*)c->off.p, c->results.p, c->seg_rem.p, c->seg_win.p, c->seq_bytes.p, SB);
    PRED_HIP(hipEventRecord(c->ev[3], st));
    // (4) the gathers
    hipLaunchKernelGGL((k_bat_gather<REM_GROUP, false, Seg64>), dim3(grid_of(2 * n * REM_GROUP)), dim3(BLOCK), 0, st, (const Seg64*)c->seg_rem.p, 2 * n,
                       (const uint8_t*)t->rem.p, t->rem_len, c->seq_bytes.p, SB);
    hipLaunchKernelGGL((k_bat_gather<WINDOW_GROUP, false, Seg64>), dim3(grid_of(2 * n * WINDOW_GROUP)), dim3(BLOCK), 0, st, (const Seg64*)c->seg_win.p, 2 * n,
                       (const uint8_t*)t->windows->bytes.p, t->windows->bytes_len, c->seq_bytes.p, SB);
    PRED_HIP(hipEventRecord(c->ev[4], st));
    PRED_HIP(hipStreamSynchronize(st));
    PRED_HIP(hipGetLastError());
    c->n_results = n;
    c->seq_bytes_len = SB;
    c->predicted = true;
    c->timing.plan_ms = hiphost::elapsed(c->ev[1], c->ev[2]);
    c->timing.scan_ms = hiphost::elapsed(c->ev[2], c->ev[3]);
    c->timing.gather_ms = hiphost::elapsed(c->ev[3], c->ev[4]);
    c->timing.seq_bytes = SB;
    return DSA_OK;
}

// groups: host memory (on_device false) or memory of `groups_device_ordinal`
int predict(const char* what, pred_ctx* c, const pred_tasks* t, const eval_group* groups, bool on_device, int64_t n, int groups_device_ordinal)
{
    if (!c || !t) return PRED_FAIL(DSA_E_ARG, "%s: no %s", what, !c ? "ctx" : "tasks");
    if (n < 0) return PRED_FAIL(DSA_E_ARG, "%s: negative number of groups (%lld)", what, (long long)n);
    if (n > (int64_t)INT32_MAX / 2) return PRED_FAIL(DSA_E_LIMIT, "%s: more than 2^30 - 1 groups in one call", what);
    if (n && !groups) return PRED_FAIL(DSA_E_ARG, "%s: no groups", what);
    if (c->device != t->device || (on_device && c->device != groups_device_ordinal))
        return PRED_FAIL(DSA_E_ARG, "%s: ctx, tasks and groups are on devices %d, %d and %d", what, c->device, t->device,
                         on_device ? groups_device_ordinal : c->device);
    c->n_results = c->seq_bytes_len = 0;
    c->predicted = false;
    c->timing = pred_timing{0, 0, 0, 0, 0, 0, n, 0};
    PRED_HIP(hipSetDevice(c->device));
    // the view of empty results has pointers too
    PRED_HIP(c->results.reserve(1));
    PRED_HIP(c->seq_bytes.reserve(4));
    if (n == 0) {
        c->predicted = true;
        return DSA_OK;
    }
    hipStream_t st = c->st;
    PRED_HIP(hipEventRecord(c->ev[0], st));
    if (!on_device) {
        PRED_HIP(c->groups.reserve((size_t)n));
        PRED_HIP(hipMemcpyAsync(c->groups.p, groups, (size_t)n * sizeof(eval_group), hipMemcpyHostToDevice, st));
        groups = c->groups.p;
    }
    PRED_HIP(hipEventRecord(c->ev[1], st));
    const int rc = predict_on_device(c, t, groups, n);
    if (rc == DSA_OK && !on_device) c->timing.upload_ms = hiphost::elapsed(c->ev[0], c->ev[1]);
    if (rc != DSA_OK) (void)hipStreamSynchronize(st);          // nothing of a refused call is in flight when it returns
    return rc;
}

}  // namespace

namespace predint {

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_pred_err = buf;
    return code;
}

void clear(pred_ctx* ctx)
{
    if (!ctx) return;
    ctx->n_results = ctx->seq_bytes_len = 0;
    ctx->predicted = false;
    ctx->timing = pred_timing{};
}

int predict_device(const char* what, pred_ctx* ctx, const pred_tasks* tasks, const eval_group* groups_device, int64_t n, int device)
{
    return predict(what, ctx, tasks, groups_device, true, n, device);
}

}  // namespace predint

extern "C" {

const char* pred_last_error(void) { return g_pred_err.c_str(); }

int pred_tasks_create(int device, const bat_windows* windows, const uint8_t* rem_bytes, int64_t rem_bytes_len, const pred_task* tasks, int64_t n,
                      pred_tasks** out)
{
    if (!out) return PRED_FAIL(DSA_E_ARG, "pred_tasks_create: no output");
    *out = nullptr;
    if (n < 0 || rem_bytes_len < 0) return PRED_FAIL(DSA_E_ARG, "negative size (%lld tasks, %lld bytes)", (long long)n, (long long)rem_bytes_len);
    if (n > (int64_t)INT32_MAX) return PRED_FAIL(DSA_E_LIMIT, "more than 2^31 - 1 tasks in one store");
    if ((n && !tasks) || (rem_bytes_len && !rem_bytes)) return PRED_FAIL(DSA_E_ARG, "pred_tasks_create: null pointer with non-zero size");
    if (!windows) return PRED_FAIL(DSA_E_ARG, "pred_tasks_create: no windows");
    std::vector<std::pair<uint32_t, int64_t>> byid((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const pred_task& t = tasks[k];
        for (int e = 0; e < 2; ++e) {
            if (t.seq_strand[e] != 0 && t.seq_strand[e] != 1)
                return PRED_FAIL(DSA_E_ARG, "task %lld: seq_strand[%d] %d is not 0 or 1", (long long)k, e, t.seq_strand[e]);
            if (t.rem_len[e] < 0) return PRED_FAIL(DSA_E_ARG, "task %lld: negative length (rem_len[%d] %d)", (long long)k, e, t.rem_len[e]);
            if (t.rem_off[e] < 0 || t.rem_off[e] > rem_bytes_len || (int64_t)t.rem_len[e] > rem_bytes_len - t.rem_off[e])
                return PRED_FAIL(DSA_E_ARG, "task %lld: remainder %d, bytes %lld + %d, is outside the %lld given", (long long)k, e, (long long)t.rem_off[e],
                                 t.rem_len[e], (long long)rem_bytes_len);
        }
        if ((int64_t)t.rem_len[0] + std::max(t.seq_len[0], 0) + 1 + std::max(t.seq_len[1], 0) + t.rem_len[1] > (int64_t)INT32_MAX)
            return PRED_FAIL(DSA_E_LIMIT, "task %lld: its longest sequence has more than 2^31 - 1 bytes", (long long)k);
        byid[(size_t)k] = {(uint32_t)t.fusion_id, k};
    }
    std::sort(byid.begin(), byid.end());
    for (int64_t s = 1; s < n; ++s)
        if (byid[(size_t)s].first == byid[(size_t)s - 1].first)
            return PRED_FAIL(DSA_E_ARG, "tasks %lld and %lld: both have fusion_id %d", (long long)byid[(size_t)s - 1].second, (long long)byid[(size_t)s].second,
                             (int32_t)byid[(size_t)s].first);
    if (hiphost::check_device(device, &g_pred_err)) return DSA_E_DEVICE;
    if (windows->device != device) return PRED_FAIL(DSA_E_ARG, "pred_tasks_create: the windows are on device %d, not %d", windows->device, device);
    PRED_HIP(hipSetDevice(device));
    pred_tasks* t = new pred_tasks();
    t->device = device;
    t->n = n;
    t->rem_len = rem_bytes_len;
    t->windows = windows;
    std::vector<uint32_t> tkey((size_t)n);
    std::vector<DevTask> task((size_t)n);
    auto build = [&]() -> int {
        if (t->st.create(hipStreamNonBlocking) != hipSuccess) return PRED_FAIL(DSA_E_DEVICE, "cannot create a stream");
        hipStream_t st = t->st;
        // the windows' ids and offsets, once: every task has to have its windows
        const int64_t W = windows->n;
        std::vector<uint32_t> wkey((size_t)W);
        std::vector<dsa_fusion> wfus((size_t)W);
        if (W) PRED_HIP(hipMemcpyAsync(wkey.data(), windows->wkey.p, (size_t)W * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (W) PRED_HIP(hipMemcpyAsync(wfus.data(), windows->wfus.p, (size_t)W * sizeof(dsa_fusion), hipMemcpyDeviceToHost, st));
        PRED_HIP(hipStreamSynchronize(st));
        for (int64_t s = 0; s < n; ++s) {
            const int64_t k = byid[(size_t)s].second;
            const pred_task& in = tasks[k];
            const auto w = std::lower_bound(wkey.begin(), wkey.end(), byid[(size_t)s].first);
            if (w == wkey.end() || *w != byid[(size_t)s].first) return PRED_FAIL(DSA_E_ARG, "task %lld: fusion_id %d has no windows", (long long)k, in.fusion_id);
            const dsa_fusion& f = wfus[(size_t)(w - wkey.begin())];
            if (std::max(in.seq_len[0], 0) != f.ref0_len || std::max(in.seq_len[1], 0) != f.ref1_len)       // (a negative seq_len: an empty window)
                return PRED_FAIL(DSA_E_ARG, "task %lld: seq_len %d, %d but its windows have %d, %d bytes", (long long)k, in.seq_len[0], in.seq_len[1], f.ref0_len,
                                 f.ref1_len);
            tkey[(size_t)s] = byid[(size_t)s].first;
            task[(size_t)s] = DevTask{{in.rem_off[0], in.rem_off[1]}, {in.rem_len[0], in.rem_len[1]}, {f.ref0_off, f.ref1_off}, {in.seq_start[0], in.seq_start[1]},
                                      {in.seq_len[0], in.seq_len[1]}, {in.seq_strand[0], in.seq_strand[1]}, {0, 0}};
        }
        PRED_HIP(t->rem.reserve((size_t)rem_bytes_len + SRC_PAD));
        PRED_HIP(t->tkey.reserve((size_t)n));
        PRED_HIP(t->task.reserve((size_t)n));
        if (rem_bytes_len) PRED_HIP(hipMemcpyAsync(t->rem.p, rem_bytes, (size_t)rem_bytes_len, hipMemcpyHostToDevice, st));
        if (n) PRED_HIP(hipMemcpyAsync(t->tkey.p, tkey.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (n) PRED_HIP(hipMemcpyAsync(t->task.p, task.data(), (size_t)n * sizeof(DevTask), hipMemcpyHostToDevice, st));
        PRED_HIP(hipStreamSynchronize(st));
        return DSA_OK;
    };
    if (const int rc = build()) {
        (void)hipStreamSynchronize(t->st);
        delete t;
        return rc;
    }
    *out = t;
    return DSA_OK;
}

void pred_tasks_destroy(pred_tasks* t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->st);
    delete t;
}

int pred_create(int device, pred_ctx** out)
{
    if (!out) return PRED_FAIL(DSA_E_ARG, "pred_create: no output");
    *out = nullptr;
    if (hiphost::check_device(device, &g_pred_err)) return DSA_E_DEVICE;
    PRED_HIP(hipSetDevice(device));
    pred_ctx* c = new pred_ctx();
    c->device = device;
    bool ok = c->st.create(hipStreamNonBlocking) == hipSuccess;
    for (auto& e : c->ev) ok = ok && e.create() == hipSuccess;
    ok = ok && c->results.reserve(1) == hipSuccess && c->seq_bytes.reserve(4) == hipSuccess;
    if (!ok) {
        delete c;
        return PRED_FAIL(DSA_E_DEVICE, "cannot create a stream or a buffer");
    }
    *out = c;
    return DSA_OK;
}

void pred_destroy(pred_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    delete c;
}

int pred_predict(pred_ctx* ctx, const pred_tasks* tasks, const eval_group* groups, int64_t n_groups)
{
    return predict("pred_predict", ctx, tasks, groups, false, n_groups, -1);
}

int pred_view(const pred_ctx* c, pred_device_view* out)
{
    if (!c || !out) return PRED_FAIL(DSA_E_ARG, "pred_view: no %s", !c ? "ctx" : "output");
    *out = pred_device_view{c->results.p, c->seq_bytes.p, c->n_results, c->seq_bytes_len, c->device, 0};
    return DSA_OK;
}

int pred_fetch(pred_ctx* c, pred_result* results, int64_t results_cap, uint8_t* seq_bytes, int64_t seq_cap)
{
    if (!c) return PRED_FAIL(DSA_E_ARG, "pred_fetch: no ctx");
    if (results_cap < 0 || seq_cap < 0) return PRED_FAIL(DSA_E_ARG, "pred_fetch: negative capacity");
    if ((results_cap && !results) || (seq_cap && !seq_bytes)) return PRED_FAIL(DSA_E_ARG, "pred_fetch: capacity without a buffer");
    if (results_cap < c->n_results || seq_cap < c->seq_bytes_len)
        return PRED_FAIL(DSA_E_CAPACITY, "the ctx has %lld results and %lld sequence bytes", (long long)c->n_results, (long long)c->seq_bytes_len);
    PRED_HIP(hipSetDevice(c->device));
    hipStream_t st = c->st;
    PRED_HIP(hipEventRecord(c->ev[5], st));
    if (c->n_results) PRED_HIP(hipMemcpyAsync(results, c->results.p, (size_t)c->n_results * sizeof(pred_result), hipMemcpyDeviceToHost, st));
    if (c->seq_bytes_len) PRED_HIP(hipMemcpyAsync(seq_bytes, c->seq_bytes.p, (size_t)c->seq_bytes_len, hipMemcpyDeviceToHost, st));
    PRED_HIP(hipEventRecord(c->ev[6], st));
    PRED_HIP(hipStreamSynchronize(st));
    c->timing.download_ms = hiphost::elapsed(c->ev[5], c->ev[6]);
    return DSA_OK;
}

int pred_get_timing(const pred_ctx* c, pred_timing* out)
{
    if (!c || !out) return PRED_FAIL(DSA_E_ARG, "pred_get_timing: no %s", !c ? "ctx" : "output");
    *out = c->timing;
    return DSA_OK;
}

}  // extern "C"
