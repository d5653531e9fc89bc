// pred_shared.hpp — what pred_api.hip gives eval_api.hip, where pred_predict_resident lives because it reads the eval_ctx:
// the prediction on groups at a device pointer, and the sink of pred_last_error(); and what it shares with task_api.hip,
// which fills a pred_tasks on the device: the task store's struct.  Internal: no part of the C ABI.
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
