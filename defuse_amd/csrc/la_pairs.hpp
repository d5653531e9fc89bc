// la_pairs.hpp — la_api.hip's third way in, for code of this library on the same device (conc_api.hip); in no public header.
#pragma once
#include <stdint.h>

#include "../../include/defuse_la.h"

// One pair: reference bytes[ref_off, + ref_len) and sequence bytes[seq_off, + seq_len) of one buffer in device memory, either
// reversed and complemented (ACGTacgt, as tools/Common.cpp) where its flag is set.
struct la_pair {
    int64_t ref_off, seq_off;
    int32_t ref_len, seq_len;
    int32_t ref_rc, seq_rc;
};

// la_align_windows_min for such pairs: `pairs` and `min_score` (or null) are host arrays, d_bytes and d_scores (n_pairs int32) device
// memory of `device`.  The pairs go up once (32 bytes each); the scores stay where the kernels store them.  The default stream is
// idle on return.  Errors as la_align_windows_min, their text in la_last_error().
__attribute__((visibility("hidden"))) int la_align_pairs_device(int device, const uint8_t* d_bytes, int64_t bytes_len, int32_t match, int32_t mismatch,
                                                                int32_t gap, const la_pair* pairs, int64_t n_pairs, const int32_t* min_score,
                                                                int32_t* d_scores, la_timing* timing);
