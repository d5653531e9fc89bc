// bat_shared.hpp — what bat_api.hip shares with pred_api.hip: the window store of bat_windows_create, which the prediction
// reads in place, and the byte gather with its segment records.  Internal: nothing here is part of the C ABI.
//
// The gather.  A group of G lanes owns a segment; lane i forms the aligned OUTPUT dword i (+ G, + 2G ...) of the segment from
// two aligned source dwords (v_alignbyte_b32), reversed with a byte permute (v_perm_b32) and complemented in registers, so a
// group stores G consecutive dwords per step.  The output is a plain concatenation: the dword in which a segment begins or
// ends also holds its neighbours' bytes, and a segment of 1, 2, 3 or 5 bytes may own no whole dword at all.  A dword store
// therefore goes only to dwords that lie wholly inside the segment; the up to three bytes before the first and after the last
// of them go out as byte stores of the same group.  No byte is written by two groups, none by a read-modify-write.
// copy_span is the plain copy for one lane; k_bat_gather without REVCOMP, and the text gathers of sct_api.hip and taskc_api.hip,
// which find their source and destination in records of their own, call it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/defuse_bat.h"
#include "hip_host.hpp"

namespace __attribute__((visibility("hidden"))) batdev {

constexpr int GATHER_BLOCK = 256;
constexpr size_t SRC_PAD = 8;         // the gather loads the aligned dword after the one a segment ends in

struct WindowsView {
    const uint32_t* wkey;       // n fusion ids, ascending as unsigned, distinct
    const dsa_fusion* wfus;     // in the same order: offsets into the windows' ref bytes
    int64_t n;
};

// one copied or reverse-complemented run of bytes of a gather
struct Seg {
    int64_t src;                // offset into the source bytes
    int32_t dst;                // offset into the output (totals are below 2^31)
    uint32_t len_rev;           // length in bits 0-30, reverse complement in bit 31
};

// the same for an output that may pass 2^31 bytes
struct Seg64 {
    int64_t src;
    int64_t dst;
    uint32_t len_rev;
    uint32_t pad_;
};

}  // namespace batdev

struct __attribute__((visibility("hidden"))) bat_windows {
    int device = -1;
    int64_t n = 0, bytes_len = 0;
    hiphost::Stream st;
    hiphost::DeviceBuffer<uint8_t> bytes;          // bytes_len + SRC_PAD
    hiphost::DeviceBuffer<uint32_t> wkey;
    hiphost::DeviceBuffer<dsa_fusion> wfus;
    batdev::WindowsView view() const { return batdev::WindowsView{wkey.p, wfus.p, n}; }
};

namespace {

// tools/Common.cpp:32-54: A<->T, C<->G in either case, every other byte value as it is.  Clearing bit 5 folds the case and
// maps no other byte onto a letter; A ^ T = 0x15, C ^ G = 0x04.
__device__ inline uint32_t complement_byte(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    const uint32_t m = (u == 0x41u || u == 0x54u) ? 0x15u : (u == 0x43u || u == 0x47u) ? 0x04u : 0u;
    return b ^ m;
}

__device__ inline uint32_t complement_word(uint32_t v)
{
    return complement_byte(v & 0xFFu) | (complement_byte((v >> 8) & 0xFFu) << 8) | (complement_byte((v >> 16) & 0xFFu) << 16) |
           (complement_byte(v >> 24) << 24);
}

// the four bytes at byte offset a of the source, from the two aligned dwords around them (the source is padded by SRC_PAD)
__device__ inline uint32_t load_word(const uint32_t* __restrict__ src, int64_t a)
{
    const uint32_t lo = src[a >> 2], hi = src[(a >> 2) + 1];
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)a & 3u);
}

// The share of lane `lane` of a group of G in the plain copy of src[s, s + len) to dst[d0, d0 + len).  The caller has checked both
// ranges; src is padded by SRC_PAD.  Returns the number of head and tail bytes: the lanes G - 1, G - 2 ... store one of them
// each, so lane G - 1 - that number is the first with none.
template <int G>
__device__ inline int64_t copy_span(const uint8_t* __restrict__ src, int64_t s, uint8_t* __restrict__ dst, int64_t d0, int64_t len, int lane)
{
    const uint32_t* __restrict__ srcw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* __restrict__ dstw = reinterpret_cast<uint32_t*>(dst);
    const int64_t d1 = d0 + len;
    // the dwords of the output that lie wholly inside [d0, d1): [w0, w1), none if w1 <= w0
    const int64_t w0 = (d0 + 3) & ~(int64_t)3, w1 = d1 & ~(int64_t)3;
    for (int64_t p = w0 + 4 * lane; p < w1; p += 4 * G) dstw[p >> 2] = load_word(srcw, s + (p - d0));
    // head [d0, h1) and tail [t0, d1): at most three bytes each, one lane per byte, from the far end of the group
    const int64_t h1 = w0 < d1 ? w0 : d1;
    const int64_t t0 = w1 > h1 ? w1 : h1;
    const int64_t nh = h1 - d0, nt = d1 - t0;
    const int64_t b = G - 1 - lane;
    if (b < nh + nt) {
        const int64_t p = b < nh ? d0 + b : t0 + (b - nh);
        dst[p] = src[s + (p - d0)];
    }
    return nh + nt;
}

// S is Seg or Seg64.  REVCOMP false: bit 31 of len_rev is ignored and the copy is copy_span.  With REVCOMP the copy stays
// written out here, with the reverse/complement branch beside the plain one: going through copy_span costs these
// instantiations one to three VGPRs (the callee is optimised on its own before it is inlined).
template <int G, bool REVCOMP = true, class S = batdev::Seg>
__global__ __launch_bounds__(batdev::GATHER_BLOCK) void k_bat_gather(const S* __restrict__ seg, int64_t n_seg, const uint8_t* __restrict__ src,
                                                                      int64_t src_len, uint8_t* __restrict__ dst, int64_t dst_len)
{
    const int64_t t = (int64_t)blockIdx.x * batdev::GATHER_BLOCK + threadIdx.x;
    const int64_t k = t / G;
    const int lane = (int)(t % G);
    if (k >= n_seg) return;
    const S s = seg[k];
    const int64_t len = (int64_t)(s.len_rev & 0x7FFFFFFFu);
    const int64_t d0 = s.dst, d1 = d0 + len;
    if (len == 0 || d0 < 0 || d1 > dst_len || s.src < 0 || s.src + len > src_len) return;
    if constexpr (!REVCOMP) (void)copy_span<G>(src, s.src, dst, d0, len, lane);
    else {
        const bool rev = (s.len_rev >> 31) != 0;
        const uint32_t* __restrict__ srcw = reinterpret_cast<const uint32_t*>(src);
        uint32_t* __restrict__ dstw = reinterpret_cast<uint32_t*>(dst);
        const int64_t w0 = (d0 + 3) & ~(int64_t)3, w1 = d1 & ~(int64_t)3;
        for (int64_t p = w0 + 4 * lane; p < w1; p += 4 * G) {
            const int64_t i = p - d0;                            // bytes i .. i + 3 of the oriented read
            uint32_t v;
            if (!rev) v = load_word(srcw, s.src + i);
            else v = complement_word(__builtin_bswap32(load_word(srcw, s.src + len - 4 - i)));  // (bswap is one v_perm_b32)
            dstw[p >> 2] = v;
        }
        const int64_t h1 = w0 < d1 ? w0 : d1;
        const int64_t t0 = w1 > h1 ? w1 : h1;
        const int64_t nh = h1 - d0, nt = d1 - t0;
        const int64_t b = G - 1 - lane;
        if (b < nh + nt) {
            const int64_t p = b < nh ? d0 + b : t0 + (b - nh);
            const int64_t i = p - d0;
            dst[p] = rev ? (uint8_t)complement_byte(src[s.src + len - 1 - i]) : src[s.src + i];
        }
    }
}

}  // namespace
