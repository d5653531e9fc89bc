// cmp_shared.hpp — what cmp_api.hip (the bin pairs) and cmpp_api.hip (the EM problems built from them) share: the binner
// object whose sorted lists the problems are built from in place, and the one last-error sink behind cmp_last_error().
#pragma once
#include <string>

#include "../../include/defuse_cmp.h"
#include "hip_host.hpp"

namespace __attribute__((visibility("hidden"))) cmpshared {

// thread-local text of cmp_last_error() (defined in cmp_api.hip)
std::string& cmp_err();

// one side (`first` or `second`) of all bin pairs after cmp_bin_run: uniq[k] the key of bin pair k (ascending, the same on
// both sides), off[k] .. off[k + 1] its list inside pay_sorted (off holds int values, n_keys + 1 of them)
struct Side {
    hiphost::DeviceBuffer<unsigned long long> key, key_sorted, uniq;
    hiphost::DeviceBuffer<cmp_packed> pay, pay_sorted;
    hiphost::DeviceBuffer<uint32_t> idx, idx_sorted, off;
    hiphost::DeviceBuffer<int> run_len;
    int64_t n = 0;
};

}  // namespace cmpshared

struct cmp_binner {
    int device = -1;
    hiphost::Stream st;
    hiphost::Event ev[2];
    int64_t n_records = 0, n_fragments = 0;
    hiphost::DeviceBuffer<cmp_record> recs;
    hiphost::DeviceBuffer<uint32_t> frag_start, cnt[4], off_first, off_second;
    hiphost::DeviceBuffer<unsigned long long> globals;
    hiphost::DeviceBuffer<uint8_t> tmp;
    hiphost::DeviceBuffer<int> n_runs;
    cmpshared::Side side[2];
    int64_t n_keys = 0;
    bool ran = false;
};
