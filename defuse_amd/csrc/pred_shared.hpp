// pred_shared.hpp — what pred_api.hip gives eval_api.hip, where pred_predict_resident lives because it reads the eval_ctx:
// the prediction on groups at a device pointer, and the sink of pred_last_error().  Internal: no part of the C ABI.
#pragma once
#include "../../include/defuse_pred.h"

namespace __attribute__((visibility("hidden"))) predint {

// printf into pred_last_error(); returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// empties the results of a ctx, as every failed prediction leaves them
void clear(pred_ctx* ctx);

// pred_predict on n groups in memory of `device`, complete when the call is made and untouched until it returns
int predict_device(const char* what, pred_ctx* ctx, const pred_tasks* tasks, const eval_group* groups_device, int64_t n, int device);

}  // namespace predint
