// pred_shared.hpp — what pred_api.hip gives eval_api.hip, where pred_predict_resident lives because it reads the eval_ctx:
// the prediction on groups at a device pointer, and the sink of pred_last_error(); and what it shares with task_api.hip,
// which fills a pred_tasks on the device: the task store's struct; and with ptext_api.hip, which prints the results of a
// pred_ctx where they lie: the ctx's struct.  Internal: no part of the C ABI.
#pragma once
#include "../../include/defuse_pred.h"
#include "bat_shared.hpp"
#include "hip_host.hpp"

namespace __attribute__((visibility("hidden"))) predint {

// a task on the device: pred_task without its id (the ids are a column of their own), with its windows' offsets
struct DevTask {
    int64_t rem_off[2];
    int32_t rem_len[2];
    int32_t win_off[2];         // of window 0 / 1 in the byte pool of bat_windows
    int32_t seq_start[2];
    int32_t seq_len[2];
    int32_t seq_strand[2];
    int32_t pad_[2];
};

// printf into pred_last_error(); returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// empties the results of a ctx, as every failed prediction leaves them
void clear(pred_ctx* ctx);

// pred_predict on n groups in memory of `device`, complete when the call is made and untouched until it returns
int predict_device(const char* what, pred_ctx* ctx, const pred_tasks* tasks, const eval_group* groups_device, int64_t n, int device);

}  // namespace predint

struct __attribute__((visibility("hidden"))) pred_tasks {
    int device = -1;
    int64_t n = 0, rem_len = 0;
    const bat_windows* windows = nullptr;
    hiphost::Stream st;
    hiphost::DeviceBuffer<uint8_t> rem;             // rem_len + SRC_PAD
    hiphost::DeviceBuffer<uint32_t> tkey;           // n fusion ids, ascending as unsigned, distinct
    hiphost::DeviceBuffer<predint::DevTask> task;   // in the same order
};

struct __attribute__((visibility("hidden"))) pred_ctx {
    using u64 = unsigned long long;
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[7];       // 0 start, 1 groups uploaded, 2 plan done, 3 descriptors done, 4 gathers done; 5, 6 around a fetch
    // the results
    bool predicted = false;     // the latest pred_predict* succeeded (its results may be empty): what ptext_format asks for
    int64_t n_results = 0, seq_bytes_len = 0;
    hiphost::DeviceBuffer<pred_result, hiphost::GrowSize> results;
    hiphost::DeviceBuffer<uint8_t, hiphost::GrowSize> seq_bytes;        // seq_bytes_len + 4: whole dwords
    // per call
    hiphost::DeviceBuffer<eval_group, hiphost::GrowSize> groups;
    hiphost::DeviceBuffer<u64, hiphost::GrowSize> len, off;
    hiphost::DeviceBuffer<uint32_t, hiphost::GrowSize> tidx;
    hiphost::DeviceBuffer<batdev::Seg64, hiphost::GrowSize> seg_rem, seg_win;
    hiphost::DeviceBuffer<uint8_t, hiphost::GrowSize> tmp;
    pred_timing timing{};
};
