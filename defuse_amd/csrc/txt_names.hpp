// txt_names.hpp — the names table text_api.hip and taskt_api.hip share: the caller's names, sorted once on the host by their
// bytes and kept in device memory, and the exact lookup of a field of a text among them (a binary search, bytes compared as
// unsigned; nothing is hashed).  Internal: nothing here is part of the C ABI.  Include hip_host.hpp first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

namespace {

struct NamesView {
    const uint8_t* bytes;
    const int64_t* off;         // n names in ascending byte order (a prefix comes first)
    const int64_t* len;
    const int32_t* index;       // the caller's number of each
    int64_t n;
};

// a and b are anything indexed by a byte position (a pointer, or a view that rewrites a byte)
template <class A, class B>
__host__ __device__ inline int compare_bytes(A a, int64_t na, B b, int64_t nb)
{
    const int64_t n = na < nb ? na : nb;
    for (int64_t k = 0; k < n; ++k) {
        const uint8_t x = a[k], y = b[k];
        if (x != y) return x < y ? -1 : 1;
    }
    return na < nb ? -1 : na > nb ? 1 : 0;
}

template <class F>
__device__ inline int32_t find_name(const NamesView& nv, F f, int64_t n)
{
    int64_t lo = 0, hi = nv.n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (compare_bytes(nv.bytes + nv.off[mid], nv.len[mid], f, n) < 0) lo = mid + 1; else hi = mid;
    }
    if (lo < nv.n && compare_bytes(nv.bytes + nv.off[lo], nv.len[lo], f, n) == 0) return nv.index[lo];
    return -1;
}

struct NameTable {
    int device = -1;
    int64_t n = 0;
    hiphost::DeviceBuffer<uint8_t> bytes;
    hiphost::DeviceBuffer<int64_t> off, len;
    hiphost::DeviceBuffer<int32_t> index;
    NamesView view() const { return NamesView{bytes.p, off.p, len.p, index.p, n}; }
};

// Name k is name_bytes[name_off[k] .. name_off[k + 1]).  The argument checks come before the device is looked at; `fn` is
// the entry point the messages name.  Fills *nm, which the caller has just made.
inline int name_table_create(std::string& err, const char* fn, int device, const uint8_t* name_bytes, int64_t name_bytes_len, const int64_t* name_off,
                             int64_t n_names, NameTable* nm)
{
    using hiphost::fail;
    if (n_names < 0 || name_bytes_len < 0) return fail(err, DSA_E_ARG, "negative size (%lld names, %lld bytes)", (long long)n_names, (long long)name_bytes_len);
    if (n_names > (int64_t)INT32_MAX) return fail(err, DSA_E_LIMIT, "more than 2^31 - 1 names");
    if ((n_names && !name_off) || (name_bytes_len && !name_bytes)) return fail(err, DSA_E_ARG, "%s: null pointer with non-zero size", fn);
    for (int64_t k = 0; k < n_names; ++k) {
        if (name_off[k] < 0 || name_off[k] > name_bytes_len) return fail(err, DSA_E_ARG, "name %lld: begins outside the %lld bytes given", (long long)k, (long long)name_bytes_len);
        if (name_off[k + 1] < name_off[k]) return fail(err, DSA_E_ARG, "name %lld: its offsets do not ascend (reversed)", (long long)k);
        if (name_off[k + 1] > name_bytes_len) return fail(err, DSA_E_ARG, "name %lld: ends outside the %lld bytes given", (long long)k, (long long)name_bytes_len);
    }
    std::vector<int32_t> order((size_t)n_names);
    std::iota(order.begin(), order.end(), 0);
    auto cmp = [&](int32_t a, int32_t b) {
        return compare_bytes(name_bytes + name_off[a], name_off[a + 1] - name_off[a], name_bytes + name_off[b], name_off[b + 1] - name_off[b]);
    };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const int c = cmp(a, b);
        return c ? c < 0 : a < b;
    });
    for (int64_t s = 1; s < n_names; ++s)
        if (cmp(order[(size_t)s - 1], order[(size_t)s]) == 0) return fail(err, DSA_E_ARG, "names %d and %d are equal", order[(size_t)s - 1], order[(size_t)s]);
    if (hiphost::check_device(device, &err)) return DSA_E_DEVICE;
    HIPHOST_TRY(err, hipSetDevice(device));
    std::vector<int64_t> off((size_t)n_names), len((size_t)n_names);
    for (int64_t s = 0; s < n_names; ++s) {
        off[(size_t)s] = name_off[order[(size_t)s]];
        len[(size_t)s] = name_off[order[(size_t)s] + 1] - name_off[order[(size_t)s]];
    }
    nm->device = device;
    nm->n = n_names;
    HIPHOST_TRY(err, nm->bytes.reserve((size_t)name_bytes_len));
    HIPHOST_TRY(err, nm->off.reserve((size_t)n_names));
    HIPHOST_TRY(err, nm->len.reserve((size_t)n_names));
    HIPHOST_TRY(err, nm->index.reserve((size_t)n_names));
    if (name_bytes_len) HIPHOST_TRY(err, hipMemcpy(nm->bytes.p, name_bytes, (size_t)name_bytes_len, hipMemcpyHostToDevice));
    if (n_names) {
        HIPHOST_TRY(err, hipMemcpy(nm->off.p, off.data(), (size_t)n_names * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPHOST_TRY(err, hipMemcpy(nm->len.p, len.data(), (size_t)n_names * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPHOST_TRY(err, hipMemcpy(nm->index.p, order.data(), (size_t)n_names * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return DSA_OK;
}

}  // namespace
