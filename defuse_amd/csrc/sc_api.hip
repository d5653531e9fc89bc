// sc_api.hip — greedy set cover on gfx950 (include/defuse_sc.h), replacing SetCover() of
// tools/setcover.cpp:30-110.  Integer/byte work: radix sort + component labelling are HBM-bound, the
// per-component greedy is latency-bound; nothing here is shaped into a GEMM.  The kernels and the run over
// clusters in device memory are sc_shared.hpp's (sct_api.hip builds its clusters there); this file is the
// host-pointer entry around them.
#include <hip/hip_runtime.h>

#include "hip_host.hpp"
#include "sc_shared.hpp"

#include <string>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_sc.h"

namespace {

using hiphost::DeviceBuffer;

thread_local std::string g_err;    // sc_prepare runs on a helper thread beside the caller's sc_cover (tools_src/setcover.cpp)

#define SC_HIP(call) HIPHOST_TRY(g_err, call)

}  // namespace

extern "C" const char* sc_last_error(void) { return g_err.c_str(); }

extern "C" int sc_prepare(int device)
{
    if (hiphost::check_device(device) || hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess) return DSA_E_DEVICE;
    return DSA_OK;
}

extern "C" int sc_cover(int device, const int64_t* cluster_off, const int32_t* elements, int32_t n_clusters,
                        int32_t max_element, int32_t* owner, sc_timing* timing)
{
    sc_timing t{};
    if (n_clusters < 0 || max_element < -1 || (n_clusters && !cluster_off)) { g_err = "bad arguments"; return DSA_E_ARG; }
    const int64_t n_occ = n_clusters ? cluster_off[n_clusters] : 0;
    for (int64_t k = 0; k < n_occ; ++k)
        if (elements[k] < 0 || elements[k] > max_element) { g_err = "element out of range"; return DSA_E_ARG; }
    if (n_occ >= ((int64_t)1 << 31)) { g_err = "more than 2^31-1 cluster lines"; return DSA_E_LIMIT; }
    if (hiphost::check_device(device, &g_err)) return DSA_E_DEVICE;
    SC_HIP(hipSetDevice(device));
    for (int64_t e = 0; e <= max_element; ++e) owner[e] = -1;
    if (n_clusters == 0 || n_occ == 0) { if (timing) *timing = t; return DSA_OK; }

    DeviceBuffer<int64_t> d_coff;
    DeviceBuffer<int32_t> d_el, d_owner;
    const int nel = max_element + 1;
    SC_HIP(d_coff.reserve(n_clusters + 1)); SC_HIP(d_el.reserve(n_occ)); SC_HIP(d_owner.reserve(nel));
    SC_HIP(hipMemcpy(d_coff.p, cluster_off, (n_clusters + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    SC_HIP(hipMemcpy(d_el.p, elements, n_occ * sizeof(int32_t), hipMemcpyHostToDevice));
    if (const int rc = sc_cover_device(g_err, nullptr, d_coff.p, d_el.p, n_clusters, n_occ, max_element, d_owner.p, t)) return rc;
    SC_HIP(hipMemcpy(owner, d_owner.p, nel * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (timing) *timing = t;
    return DSA_OK;
}
