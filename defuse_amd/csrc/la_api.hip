// la_api.hip — batched SimpleAligner scores on gfx950 behind the C ABI of include/defuse_la.h.
//
// Layout mirrors the split-read DP (dsa_kernels.hpp): a lane owns its pairs for the whole matrix, the
// reference is cut into tiles of W = 64 columns that live in registers, rows stream through, and the
// last column of a tile is handed to the next tile through a per-wave plane in HBM (two planes,
// ping-pong).  Four consecutive rows of a lane share one 16-byte word of every plane.
//
//   k_la16: two pairs per lane (lo / hi 16-bit fields).  Works on Y = H - gap*j (>= 0, kept biased so
//           that every field is the bit pattern of a positive normal fp16 and v_pk_maximum3_f16 is an
//           exact integer maximum, as in dsa_kernels.hpp):
//               Y(i,j) = max3(Y(i-1,j-1) + s - gap, Y(i,j-1), Y(i-1,j) + gap)
//           per column: xor + pk_min + pk_mad (score term), add (diagonal), sub (left), max3, and half a
//           max3 for the row maximum.  Needs gap <= mismatch <= 0 and a bounded value range.
//           With a minimum score per pair (the tool's -t threshold) it prunes exactly, as the split-read fill
//           does: a cell with H + max(match,0)*(rows left) < need cannot lie on the path to a score >= need, so
//           once a whole row group of a tile and the boundary entering it are dead the tile is left.
//           Every wave adds the row groups it swept (over its tiles) to one 64-bit counter: la_timing.row_groups16.
//   k_la32: one pair per lane in int32, any scores, padded columns masked out of the maximum.
//
// Pairs are sorted by (sequence length, reference length) so that the lanes of a wave sweep about the
// same number of rows and tiles.
//
// Two ways in: la_align_batch_min takes references and sequences from one host pool (k_pack fills the codes);
// la_align_windows_min (matealign) cuts every reference out of a genome kept in HBM by la_genome_create, from a
// 40-byte descriptor per pair (k_pack_win).  A third, la_align_pairs_device (la_pairs.hpp, for conc_api.hip), takes both sides of a
// pair from sequence bytes in HBM, each with its own reverse-complement flag (k_pack_pairs), and leaves the scores on the device.
// All run the same launch groups and the same two kernels.
#include <hip/hip_runtime.h>

#include "hip_host.hpp"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/defuse_dsa.h"
#include "../../include/defuse_la.h"
#include "la_pairs.hpp"

namespace la {

constexpr int W = 64;
constexpr int WAVE = 64;
constexpr int WG_WAVES = 4;
constexpr uint32_t REF_PAD = 0x0100u;      // never equals a byte nor ROW_PAD
constexpr uint32_t ROW_PAD = 0x0200u;
constexpr uint32_t BIAS16 = 0x0800u;       // Y = 0
constexpr uint32_t BIAS2 = BIAS16 * 0x00010001u;
constexpr int Y_LIMIT = 30000;             // largest biased value the packed kernel may reach (< 0x7C00)

typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef unsigned short v2u __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t max3(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_maximum(
                                            __builtin_elementwise_maximum(__builtin_bit_cast(v2h, a), __builtin_bit_cast(v2h, b)),
                                            __builtin_bit_cast(v2h, c)));
}

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)   // per-field unsigned maximum
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(v2u, a), __builtin_bit_cast(v2u, b)));
}

struct Lane {              // what one lane aligns: ITEMS pairs (second one unused by the int32 kernel)
    int32_t lr[2], ls[2];
    int32_t out[2];        // index into scores, -1 = padding
    int32_t need[2];       // scores below this need not be exact (NO_NEED: always exact)
};
constexpr int32_t NO_NEED = -0x40000000;
struct Wave {
    int64_t ref_off;       // dwords into refcodes: [nch*W columns][64 lanes]
    int64_t row_off;       // dwords into rowcodes: [rows4][64 lanes], rowidx layout
    int64_t bnd_off;       // dwords into bnd: 2 planes of [rows4][64 lanes]
    int32_t nch, ls_max, rows4, pad_;
};
struct Params {
    int32_t match, mismatch, gap;      // as given (int32 kernel)
    int32_t dm, dx, gd;                // packed kernel: match - gap, mismatch - gap (after the 2*gap clamp), -gap
    int32_t mp;                        // max(match, 0): the most a further row can add to a score
};

__host__ __device__ __forceinline__ int64_t rowidx(int j, int lane) { return ((int64_t)(j >> 2) * WAVE + lane) * 4 + (j & 3); }

// codes of both planes; ITEMS pairs per lane share a dword (16 bits each)
template <int ITEMS>
__global__ void k_pack(const uint8_t* __restrict__ pool, const la_item* __restrict__ items, const Lane* __restrict__ lanes,
                       const Wave* __restrict__ waves, uint32_t* __restrict__ refcodes, uint32_t* __restrict__ rowcodes)
{
    const int w = blockIdx.x;
    const Wave wv = waves[w];
    const int lane = threadIdx.x & 63;
    const Lane ln = lanes[(int64_t)w * WAVE + lane];
    const uint8_t* ref[2] = {nullptr, nullptr};
    const uint8_t* seq[2] = {nullptr, nullptr};
#pragma unroll
    for (int f = 0; f < ITEMS; ++f)
        if (ln.out[f] >= 0) {
            ref[f] = pool + items[ln.out[f]].ref_off;
            seq[f] = pool + items[ln.out[f]].seq_off;
        }
    for (int i = threadIdx.x >> 6; i < wv.nch * W; i += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f) code |= ((ref[f] != nullptr && i < ln.lr[f]) ? (uint32_t)ref[f][i] : REF_PAD) << (16 * f);
        refcodes[wv.ref_off + (int64_t)i * WAVE + lane] = code;
    }
    for (int j = threadIdx.x >> 6; j < wv.rows4; j += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f)
            code |= ((seq[f] != nullptr && j >= 1 && j <= ln.ls[f]) ? (uint32_t)seq[f][j - 1] : ROW_PAD) << (16 * f);
        rowcodes[wv.row_off + rowidx(j, lane)] = code;
    }
}

__device__ __forceinline__ uint32_t complement(uint32_t b)     // tools/Common.cpp:32-54: ACGTacgt only
{
    const uint32_t up = b & ~0x20u;
    const uint32_t c = up == 'A' ? 'T' : up == 'T' ? 'A' : up == 'C' ? 'G' : up == 'G' ? 'C' : 0u;
    return c ? (c | (b & 0x20u)) : b;
}

// k_pack for windows cut from a genome in HBM (la_align_windows_min): the reference of a pair is
// 'N' x pad_left + genome[slice_off, + slice_len) + 'N' x pad_right, reversed and complemented when revcomp is set
template <int ITEMS>
__global__ void k_pack_win(const uint8_t* __restrict__ genome, const uint8_t* __restrict__ pool, const la_window* __restrict__ wins,
                           const Lane* __restrict__ lanes, const Wave* __restrict__ waves, uint32_t* __restrict__ refcodes,
                           uint32_t* __restrict__ rowcodes)
{
    const int w = blockIdx.x;
    const Wave wv = waves[w];
    const int lane = threadIdx.x & 63;
    const Lane ln = lanes[(int64_t)w * WAVE + lane];
    const uint8_t* slice[2] = {nullptr, nullptr};
    const uint8_t* seq[2] = {nullptr, nullptr};
    int32_t pl[2] = {0, 0}, sl[2] = {0, 0}, rc[2] = {0, 0};
#pragma unroll
    for (int f = 0; f < ITEMS; ++f)
        if (ln.out[f] >= 0) {
            const la_window wd = wins[ln.out[f]];
            slice[f] = genome + wd.slice_off;
            seq[f] = pool + wd.seq_off;
            pl[f] = wd.pad_left;
            sl[f] = wd.slice_len;
            rc[f] = wd.revcomp;
        }
    for (int i = threadIdx.x >> 6; i < wv.nch * W; i += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f) {
            uint32_t c = REF_PAD;
            if (slice[f] != nullptr && i < ln.lr[f]) {
                const int q = (rc[f] ? ln.lr[f] - 1 - i : i) - pl[f];          // byte of the window before reversal
                c = (q >= 0 && q < sl[f]) ? (uint32_t)slice[f][q] : (uint32_t)'N';
                if (rc[f]) c = complement(c);
            }
            code |= c << (16 * f);
        }
        refcodes[wv.ref_off + (int64_t)i * WAVE + lane] = code;
    }
    for (int j = threadIdx.x >> 6; j < wv.rows4; j += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f)
            code |= ((seq[f] != nullptr && j >= 1 && j <= ln.ls[f]) ? (uint32_t)seq[f][j - 1] : ROW_PAD) << (16 * f);
        rowcodes[wv.row_off + rowidx(j, lane)] = code;
    }
}

// k_pack for pairs whose reference and sequence are both slices of bytes in HBM (la_align_pairs_device): either side is reversed
// and complemented in the gather where its flag is set
template <int ITEMS>
__global__ void k_pack_pairs(const uint8_t* __restrict__ bytes, const la_pair* __restrict__ pairs, const Lane* __restrict__ lanes,
                             const Wave* __restrict__ waves, uint32_t* __restrict__ refcodes, uint32_t* __restrict__ rowcodes)
{
    const int w = blockIdx.x;
    const Wave wv = waves[w];
    const int lane = threadIdx.x & 63;
    const Lane ln = lanes[(int64_t)w * WAVE + lane];
    const uint8_t* ref[2] = {nullptr, nullptr};
    const uint8_t* seq[2] = {nullptr, nullptr};
    int32_t rrc[2] = {0, 0}, src[2] = {0, 0};
#pragma unroll
    for (int f = 0; f < ITEMS; ++f)
        if (ln.out[f] >= 0) {
            const la_pair pr = pairs[ln.out[f]];
            ref[f] = bytes + pr.ref_off;
            seq[f] = bytes + pr.seq_off;
            rrc[f] = pr.ref_rc;
            src[f] = pr.seq_rc;
        }
    for (int i = threadIdx.x >> 6; i < wv.nch * W; i += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f) {
            uint32_t c = REF_PAD;
            if (ref[f] != nullptr && i < ln.lr[f]) c = rrc[f] ? complement((uint32_t)ref[f][ln.lr[f] - 1 - i]) : (uint32_t)ref[f][i];
            code |= c << (16 * f);
        }
        refcodes[wv.ref_off + (int64_t)i * WAVE + lane] = code;
    }
    for (int j = threadIdx.x >> 6; j < wv.rows4; j += blockDim.x >> 6) {
        uint32_t code = 0;
#pragma unroll
        for (int f = 0; f < ITEMS; ++f) {
            uint32_t c = ROW_PAD;
            if (seq[f] != nullptr && j >= 1 && j <= ln.ls[f]) c = src[f] ? complement((uint32_t)seq[f][ln.ls[f] - j]) : (uint32_t)seq[f][j - 1];
            code |= c << (16 * f);
        }
        rowcodes[wv.row_off + rowidx(j, lane)] = code;
    }
}

// ---------------------------------------------------------------------------------------------
// packed kernel: two pairs per lane
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG_WAVES * WAVE, 2) void k_la16(const Lane* __restrict__ lanes, const Wave* __restrict__ waves, int n_waves,
                                                           const uint32_t* __restrict__ refcodes,
                                                           const uint32_t* __restrict__ rowcodes, uint32_t* __restrict__ bnd,
                                                           Params prm, int32_t* __restrict__ scores,
                                                           unsigned long long* __restrict__ row_groups)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WG_WAVES + (threadIdx.x >> 6)));
    if (w >= n_waves) return;
    const int lane = threadIdx.x & 63;
    const Wave wv = waves[w];
    const Lane ln = lanes[(int64_t)w * WAVE + lane];
    const uint32_t gd2 = (uint32_t)prm.gd * 0x00010001u;
    const uint32_t dm2 = (uint32_t)prm.dm * 0x00010001u;
    const uint32_t nd2 = (uint32_t)((prm.dx - prm.dm) & 0xFFFF) * 0x00010001u;     // mod 2^16 per field
    const uint32_t one2 = 0x00010001u;
    // score term of a cell: dm where the codes are equal, dx elsewhere (per field): xor, then min(.,1) and a
    // multiply-add on both fields at once.  Written as the two packed instructions: from the C expression
    // the compiler builds per-field compares, selects and a permute (11 instructions per column instead of 7).
    auto term = [&](uint32_t r, uint32_t q) -> uint32_t {
        uint32_t t, d;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(t) : "v"(r ^ q), "v"(one2));
        asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(d) : "v"(t), "v"(nd2), "v"(dm2));
        return d;
    };
    const uint4* rows4 = reinterpret_cast<const uint4*>(rowcodes + wv.row_off) + lane;
    const int64_t plane = (int64_t)wv.rows4 * WAVE;
    const uint4 bias4 = make_uint4(BIAS2, BIAS2, BIAS2, BIAS2);
    const int ngq = (wv.ls_max >> 2) + 1;
    int best0 = 0, best1 = 0;
    // pruning: field f is alive at row j while Y (biased) >= need_f - mp*ls_f + (mp + gd)*j + BIAS
    const int slope = prm.mp + prm.gd;
    const int base0 = ln.need[0] - prm.mp * ln.ls[0] + (int)BIAS16, base1 = ln.need[1] - prm.mp * ln.ls[1] + (int)BIAS16;
    auto wave_max = [](int v) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
        return v;
    };
    auto rows_alive_at_zero = [&](int base, int ls) {          // rows at which Y = 0 (column 0, fresh starts) is alive
        if (ls <= 0) return 0;
        if (base - (int)BIAS16 <= 0 && slope <= 0) return ls;
        if (base - (int)BIAS16 > 0) return 0;
        return min(ls, ((int)BIAS16 - base) / slope);
    };
    int l_in = wave_max(max(rows_alive_at_zero(base0, ln.ls[0]), rows_alive_at_zero(base1, ln.ls[1])));
    int stop_prev = 0;
    unsigned long long swept = 0;           // row groups this wave swept, all tiles (wave-uniform)

    for (int c = 0; c < wv.nch; ++c) {
        uint32_t r[W];
        const uint32_t* rc = refcodes + wv.ref_off + (int64_t)c * W * WAVE + lane;
#pragma unroll
        for (int i = 0; i < W; ++i) r[i] = rc[(int64_t)i * WAVE];
        uint32_t X[W];
#pragma unroll
        for (int i = 0; i < W; ++i) X[i] = BIAS2;              // row 0: Y = 0
        const uint4* in4 = reinterpret_cast<const uint4*>(bnd + wv.bnd_off + ((c - 1) & 1) * plane) + lane;
        uint4* out4 = reinterpret_cast<uint4*>(bnd + wv.bnd_off + (c & 1) * plane) + lane;
        uint32_t bprev = BIAS2;
        uint4 rc_n = rows4[0];
        uint4 b_n = c == 0 ? bias4 : in4[0];                    // every tile stores at least its first row group
        int last_bnd = 0;
        int gq = 0;
        for (; gq < ngq; ++gq) {
            const uint4 rcq = rc_n, b = b_n;
            const int gn = gq + 1 < ngq ? gq + 1 : gq;
            rc_n = rows4[(int64_t)gn * WAVE];
            b_n = (c > 0 && gn < stop_prev) ? in4[(int64_t)gn * WAVE] : bias4;   // past the left tile's stop: dead, Y = 0
            const uint32_t rcv[4] = {rcq.x, rcq.y, rcq.z, rcq.w}, bv[4] = {b.x, b.y, b.z, b.w};
            uint32_t bov[4] = {BIAS2, BIAS2, BIAS2, BIAS2};
            uint32_t alive_bits = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int j = 4 * gq + s;
                const uint32_t bcur = bv[s];            // Y(c*W, j); column 0 of the matrix: H = j*gap, Y = 0
                if (j >= 1 && j <= wv.ls_max) {         // wave-uniform
                    const uint32_t q = rcv[s];
                    uint32_t a = bprev + term(r[0], q);
                    uint32_t left = bcur - gd2;
                    uint32_t m0 = BIAS2, m1 = BIAS2;
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        uint32_t an = 0;
                        if (i + 1 < W) an = X[i] + term(r[i + 1], q);
                        X[i] = max3(a, X[i], left);
                        left = X[i] - gd2;
                        a = an;
                        if (i & 1) {
                            if (i & 2) m1 = max3(m1, X[i - 1], X[i]);
                            else m0 = max3(m0, X[i - 1], X[i]);
                        }
                    }
                    // padded columns and rows never beat the true maximum here (gap, mismatch <= 0): the
                    // row maximum needs no column mask, rows past a pair's sequence are skipped
                    const uint32_t m = max3(m0, m1, BIAS2);
                    const int off = (int)BIAS16 + prm.gd * j;           // H = Y + gap*j
                    const int h0 = (int)(m & 0xFFFFu) - off, h1 = (int)(m >> 16) - off;
                    if (j <= ln.ls[0]) best0 = max(best0, h0);
                    if (j <= ln.ls[1]) best1 = max(best1, h1);
                    bov[s] = X[W - 1];
                    // alive fields: x >= thr <=> max(x, thr - 1) != thr - 1; rows past a field's sequence compare with 0xFFFF
                    const uint32_t t0 = j <= ln.ls[0] ? (uint32_t)min(max(base0 + slope * j - 1, 0), 0xFFFE) : 0xFFFFu;
                    const uint32_t t1 = j <= ln.ls[1] ? (uint32_t)min(max(base1 + slope * j - 1, 0), 0xFFFE) : 0xFFFFu;
                    const uint32_t tm2 = t0 | (t1 << 16);
                    alive_bits |= pk_max_u16(m, tm2) ^ tm2;
                    if ((pk_max_u16(bov[s], tm2) ^ tm2) != 0u) last_bnd = j;
                }
                bprev = bcur;
            }
            if (c + 1 < wv.nch) out4[(int64_t)gq * WAVE] = make_uint4(bov[0], bov[1], bov[2], bov[3]);
            // a live boundary value at row l_in also enters row l_in + 1 (diagonal move): sweep past it
            if (4 * gq + 3 > l_in && __builtin_amdgcn_ballot_w64(alive_bits != 0u) == 0) { ++gq; break; }   // wave-uniform
        }
        stop_prev = gq;
        swept += (unsigned long long)gq;
        l_in = wave_max(last_bnd);
    }
    if (lane == 0) atomicAdd(row_groups, swept);
    if (ln.out[0] >= 0) scores[ln.out[0]] = best0;
    if (ln.out[1] >= 0) scores[ln.out[1]] = best1;
}

// ---------------------------------------------------------------------------------------------
// int32 kernel: one pair per lane, any scores
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG_WAVES * WAVE) void k_la32(const Lane* __restrict__ lanes, const Wave* __restrict__ waves, int n_waves,
                                                         const uint32_t* __restrict__ refcodes,
                                                         const uint32_t* __restrict__ rowcodes, uint32_t* __restrict__ bnd,
                                                         Params prm, int32_t* __restrict__ scores)
{
    const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WG_WAVES + (threadIdx.x >> 6)));
    if (w >= n_waves) return;
    const int lane = threadIdx.x & 63;
    const Wave wv = waves[w];
    const Lane ln = lanes[(int64_t)w * WAVE + lane];
    const int64_t plane = (int64_t)wv.rows4 * WAVE;
    const uint32_t* rows = rowcodes + wv.row_off;
    int best = 0;
    for (int c = 0; c < wv.nch; ++c) {
        uint32_t r[W];
        const uint32_t* rc = refcodes + wv.ref_off + (int64_t)c * W * WAVE + lane;
#pragma unroll
        for (int i = 0; i < W; ++i) r[i] = rc[(int64_t)i * WAVE];
        int X[W];
#pragma unroll
        for (int i = 0; i < W; ++i) X[i] = 0;                  // H(i,0) = 0
        const int nv = min(W, max(0, ln.lr[0] - c * W));        // columns of this tile that exist
        const int* in = reinterpret_cast<const int*>(bnd + wv.bnd_off + ((c - 1) & 1) * plane);
        int* out = reinterpret_cast<int*>(bnd + wv.bnd_off + (c & 1) * plane);
        int bprev = 0;
        for (int j = 1; j <= wv.ls_max; ++j) {                  // wave-uniform
            const uint32_t q = rows[rowidx(j, lane)];
            const int bcur = c == 0 ? j * prm.gap : in[rowidx(j, lane)];
            int a = bprev + (r[0] == q ? prm.match : prm.mismatch);
            int left = bcur + prm.gap;
            const bool count = j <= ln.ls[0];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                int an = 0;
                if (i + 1 < W) an = X[i] + (r[i + 1] == q ? prm.match : prm.mismatch);
                X[i] = max(a, max(X[i] + prm.gap, left));
                left = X[i] + prm.gap;
                a = an;
                if (count && i < nv) best = max(best, X[i]);
            }
            if (c + 1 < wv.nch) out[rowidx(j, lane)] = X[W - 1];
            bprev = bcur;
        }
    }
    if (ln.out[0] >= 0) scores[ln.out[0]] = best;
}

}  // namespace la

struct la_genome {             // include/defuse_la.h: the contig bytes of a genome in HBM
    int device;
    hiphost::DeviceBuffer<uint8_t> bytes;
    int64_t len;
};

namespace {

using namespace la;

using hiphost::DeviceBuffer;
using hiphost::fail;

thread_local std::string g_err;

#define HIPL(call) HIPHOST_TRY(g_err, call)

// One launch group: the waves built from `order[begin..end)`, ITEMS pairs per lane.
struct Group {
    std::vector<Lane> lanes;
    std::vector<Wave> waves;
    int64_t ref_dwords = 0, row_dwords = 0, bnd_dwords = 0;
};

inline int32_t ref_len(const la_item& it) { return it.ref_len; }
inline int32_t ref_len(const la_window& wd) { return wd.pad_left + wd.slice_len + wd.pad_right; }
inline int32_t ref_len(const la_pair& pr) { return pr.ref_len; }

template <class Item>
void add_wave(Group& g, const Params& prm, const Item* items, const int32_t* min_score, const int64_t* order, int64_t n, int items_per_lane)
{
    Wave wv{};
    wv.ref_off = g.ref_dwords;
    wv.row_off = g.row_dwords;
    wv.bnd_off = g.bnd_dwords;
    int lr_max = 0, ls_max = 0;
    for (int lane = 0; lane < WAVE; ++lane) {
        Lane ln{};
        for (int f = 0; f < 2; ++f) {
            ln.out[f] = -1;
            ln.need[f] = NO_NEED;
            const int64_t k = (int64_t)lane * items_per_lane + f;
            if (f < items_per_lane && k < n) {
                const Item& it = items[order[k]];
                ln.out[f] = (int32_t)order[k];
                ln.lr[f] = ref_len(it);
                ln.ls[f] = it.seq_len;
                if (min_score) {
                    // no score exceeds mp * seq_len: a minimum above it is as unreachable one above it, and the kernel's
                    // thresholds (need - mp*ls + slope*j + BIAS) then stay far inside int
                    const int64_t top = (int64_t)prm.mp * it.seq_len + 1;
                    ln.need[f] = (int32_t)std::max<int64_t>(std::min<int64_t>(min_score[order[k]], top), NO_NEED);
                }
                lr_max = std::max(lr_max, ln.lr[f]);
                ls_max = std::max(ls_max, it.seq_len);
            }
        }
        g.lanes.push_back(ln);
    }
    wv.nch = (lr_max + W - 1) / W;
    wv.ls_max = ls_max;
    wv.rows4 = (ls_max + 1 + 3) & ~3;
    g.ref_dwords += (int64_t)wv.nch * W * WAVE;
    g.row_dwords += (int64_t)wv.rows4 * WAVE;
    g.bnd_dwords += 2 * (int64_t)wv.rows4 * WAVE;
    g.waves.push_back(wv);
}

// Everything after the checks of the entry points: the 16-bit / int32 split, launch groups within the scratch budget, and per
// group the pack step, then k_la16 or k_la32.  The items (la_item or la_window) and the pool go to the device as given;
// pack(items_per_lane, n_waves, d_pool, d_items, d_lanes, d_waves, d_ref, d_row) launches the step that fills a group's codes.
// With d_scores_out (n_items int32 in device memory) the kernels store there and nothing comes down into `scores`.
template <class Item, class Pack>
int align_items(int device, int32_t match, int32_t mismatch, int32_t gap, const uint8_t* pool, int64_t pool_len, const Item* items,
                int64_t n_items, const int32_t* min_score, int32_t* scores, la_timing& tm, Pack pack, int32_t* d_scores_out = nullptr)
{
    if (n_items == 0) return DSA_OK;
    HIPL(hipSetDevice(device));

    // Moves by mismatch are never better than two gaps when mismatch < 2*gap (same for match): clamping
    // gives the same matrix and keeps the packed kernel's diagonal term non-negative.
    Params prm{};
    prm.match = match;
    prm.mismatch = mismatch;
    prm.gap = gap;
    prm.gd = -gap;
    prm.dm = std::max(match, 2 * gap) - gap;
    prm.dx = std::max(mismatch, 2 * gap) - gap;
    prm.mp = std::max(match, 0);

    // longest sequences first; a wave takes consecutive pairs
    std::vector<int64_t> order((size_t)n_items);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (items[a].seq_len != items[b].seq_len) return items[a].seq_len > items[b].seq_len;
        if (ref_len(items[a]) != ref_len(items[b])) return ref_len(items[a]) > ref_len(items[b]);
        return a < b;
    });
    // the packed kernel takes the pairs whose values fit 16-bit fields
    const bool scores16 = gap <= 0 && mismatch <= 0 && prm.gd <= 1000 && prm.dm >= 0 && prm.dm <= 1000 && prm.dx >= 0 && prm.dx <= 1000;
    const int64_t step = std::max(prm.dm, std::max(prm.dx, 1));
    int64_t first16 = n_items;      // order[first16..) go to the packed kernel (sequence lengths descend)
    if (scores16) {
        first16 = 0;
        while (first16 < n_items && (int64_t)BIAS16 + (int64_t)items[order[first16]].seq_len * step > Y_LIMIT) ++first16;
    }
    tm.n_int32 = (int32_t)first16;
    tm.n_packed16 = (int32_t)(n_items - first16);

    DeviceBuffer<uint8_t> d_pool;
    DeviceBuffer<Item> d_items;
    DeviceBuffer<int32_t> d_scores;
    DeviceBuffer<unsigned long long> d_row_groups;      // what k_la16 swept in this call
    HIPL(d_pool.reserve((size_t)pool_len));
    HIPL(d_items.reserve((size_t)n_items));
    if (!d_scores_out) HIPL(d_scores.reserve((size_t)n_items));
    int32_t* const d_scores_p = d_scores_out ? d_scores_out : d_scores.p;
    HIPL(d_row_groups.reserve(1));
    HIPL(hipMemset(d_row_groups.p, 0, sizeof(unsigned long long)));
    if (pool_len > 0) HIPL(hipMemcpy(d_pool.p, pool, (size_t)pool_len, hipMemcpyHostToDevice));
    HIPL(hipMemcpy(d_items.p, items, (size_t)n_items * sizeof(Item), hipMemcpyHostToDevice));
    hiphost::Event ev[3];                 // destroyed on every return
    for (auto& e : ev) HIPL(e.create());

    size_t budget_dwords = (size_t)2 << 28;       // 2 GiB of planes per launch group
    if (const char* e = getenv("DEFUSE_LA_SCRATCH_MB")) budget_dwords = std::max<size_t>(1, (size_t)atoll(e)) << 18;

    auto run_range = [&](int64_t begin, int64_t end, int items_per_lane) -> int {
        const int64_t per_wave = (int64_t)WAVE * items_per_lane;
        int64_t k = begin;
        while (k < end) {
            Group g;
            while (k < end) {
                const int64_t n = std::min(per_wave, end - k);
                add_wave(g, prm, items, min_score, order.data() + k, n, items_per_lane);
                k += n;
                if ((size_t)(g.ref_dwords + g.row_dwords + g.bnd_dwords) >= budget_dwords) break;
            }
            DeviceBuffer<Lane> d_lanes;
            DeviceBuffer<Wave> d_waves;
            DeviceBuffer<uint32_t> d_ref, d_row, d_bnd;
            HIPL(d_lanes.reserve(g.lanes.size()));
            HIPL(d_waves.reserve(g.waves.size()));
            HIPL(d_ref.reserve((size_t)g.ref_dwords));
            HIPL(d_row.reserve((size_t)g.row_dwords));
            HIPL(d_bnd.reserve((size_t)g.bnd_dwords));
            HIPL(hipMemcpy(d_lanes.p, g.lanes.data(), g.lanes.size() * sizeof(Lane), hipMemcpyHostToDevice));
            HIPL(hipMemcpy(d_waves.p, g.waves.data(), g.waves.size() * sizeof(Wave), hipMemcpyHostToDevice));
            const int n_waves = (int)g.waves.size();
            HIPL(hipEventRecord(ev[0], nullptr));
            pack(items_per_lane, n_waves, d_pool.p, d_items.p, d_lanes.p, d_waves.p, d_ref.p, d_row.p);
            HIPL(hipEventRecord(ev[1], nullptr));
            const unsigned grid = hiphost::grid_of(n_waves, WG_WAVES);
            if (items_per_lane == 2)
                hipLaunchKernelGGL(k_la16, dim3(grid), dim3(WG_WAVES * WAVE), 0, nullptr, d_lanes.p, d_waves.p, n_waves, d_ref.p, d_row.p,
                                   d_bnd.p, prm, d_scores_p, d_row_groups.p);
            else
                hipLaunchKernelGGL(k_la32, dim3(grid), dim3(WG_WAVES * WAVE), 0, nullptr, d_lanes.p, d_waves.p, n_waves, d_ref.p, d_row.p,
                                   d_bnd.p, prm, d_scores_p);
            HIPL(hipEventRecord(ev[2], nullptr));
            HIPL(hipEventSynchronize(ev[2]));
            HIPL(hipGetLastError());
            float ms = 0;
            HIPL(hipEventElapsedTime(&ms, ev[0], ev[1]));
            tm.pack_ms += ms;
            HIPL(hipEventElapsedTime(&ms, ev[1], ev[2]));
            tm.kernel_ms += ms;
        }
        return DSA_OK;
    };
    int rc = run_range(0, first16, 1);
    if (rc == DSA_OK) rc = run_range(first16, n_items, 2);
    if (rc != DSA_OK) return rc;
    if (!d_scores_out) HIPL(hipMemcpy(scores, d_scores.p, (size_t)n_items * sizeof(int32_t), hipMemcpyDeviceToHost));
    unsigned long long row_groups = 0;
    HIPL(hipMemcpy(&row_groups, d_row_groups.p, sizeof row_groups, hipMemcpyDeviceToHost));
    tm.row_groups16 = (int32_t)std::min<unsigned long long>(row_groups, (unsigned long long)INT32_MAX);
    return DSA_OK;
}

}  // namespace

extern "C" {

const char* la_last_error(void) { return g_err.c_str(); }

int la_align_batch(int device, int32_t match, int32_t mismatch, int32_t gap, const uint8_t* pool, int64_t pool_len,
                   const la_item* items, int64_t n_items, int32_t* scores, la_timing* timing)
{
    return la_align_batch_min(device, match, mismatch, gap, pool, pool_len, items, n_items, nullptr, scores, timing);
}

int la_align_batch_min(int device, int32_t match, int32_t mismatch, int32_t gap, const uint8_t* pool, int64_t pool_len,
                       const la_item* items, int64_t n_items, const int32_t* min_score, int32_t* scores, la_timing* timing)
{
    const auto t_begin = std::chrono::steady_clock::now();
    la_timing tm{};
    if (n_items < 0 || (n_items > 0 && (!items || !scores || !pool))) return fail(g_err, DSA_E_ARG, "null argument");
    if (n_items >= (int64_t)1 << 31) return fail(g_err, DSA_E_LIMIT, "more than 2^31-1 pairs");
    for (int64_t k = 0; k < n_items; ++k) {
        const la_item& it = items[k];
        if (it.ref_len < 0 || it.seq_len < 0 || it.ref_off < 0 || it.seq_off < 0 || it.ref_off + it.ref_len > pool_len ||
            it.seq_off + it.seq_len > pool_len)
            return fail(g_err, DSA_E_ARG, "pair %lld lies outside the pool", (long long)k);
        tm.cells += ((int64_t)it.ref_len + 1) * ((int64_t)it.seq_len + 1);
    }
    if (n_items == 0) {
        if (timing) *timing = tm;
        return DSA_OK;
    }
    const int rc = align_items(device, match, mismatch, gap, pool, pool_len, items, n_items, min_score, scores, tm,
                               [](int items_per_lane, int n_waves, const uint8_t* d_pool, const la_item* d_items, const Lane* d_lanes,
                                  const Wave* d_waves, uint32_t* d_ref, uint32_t* d_row) {
                                   if (items_per_lane == 2)
                                       hipLaunchKernelGGL(k_pack<2>, dim3(n_waves), dim3(256), 0, nullptr, d_pool, d_items, d_lanes, d_waves, d_ref, d_row);
                                   else
                                       hipLaunchKernelGGL(k_pack<1>, dim3(n_waves), dim3(256), 0, nullptr, d_pool, d_items, d_lanes, d_waves, d_ref, d_row);
                               });
    if (rc != DSA_OK) return rc;
    tm.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (timing) *timing = tm;
    return DSA_OK;
}

int la_genome_create(int device, const uint8_t* bytes, int64_t len, la_genome** out)
{
    if (!out || len < 0 || (len > 0 && !bytes)) return fail(g_err, DSA_E_ARG, "null argument");
    *out = nullptr;
    HIPL(hipSetDevice(device));
    DeviceBuffer<uint8_t> d;           // freed on the early returns
    HIPL(d.reserve((size_t)len));
    if (len > 0) {
        const hipError_t e = hipMemcpy(d.p, bytes, (size_t)len, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(g_err, DSA_E_DEVICE, "hipMemcpy of the genome: %s", hipGetErrorString(e));
    }
    *out = new la_genome{device, {}, len};
    (*out)->bytes.swap(d);
    return DSA_OK;
}

void la_genome_destroy(la_genome* genome)
{
    if (!genome) return;
    (void)hipSetDevice(genome->device);
    delete genome;
}

int la_align_windows_min(const la_genome* genome, int32_t match, int32_t mismatch, int32_t gap, const uint8_t* pool, int64_t pool_len,
                         const la_window* windows, int64_t n_windows, const int32_t* min_score, int32_t* scores, la_timing* timing)
{
    const auto t_begin = std::chrono::steady_clock::now();
    la_timing tm{};
    if (!genome || n_windows < 0 || (n_windows > 0 && (!windows || !scores || (!pool && pool_len > 0)))) return fail(g_err, DSA_E_ARG, "null argument");
    if (n_windows >= (int64_t)1 << 31) return fail(g_err, DSA_E_LIMIT, "more than 2^31-1 pairs");
    for (int64_t k = 0; k < n_windows; ++k) {
        const la_window& wd = windows[k];
        const int64_t lr = (int64_t)wd.pad_left + wd.slice_len + wd.pad_right;
        if (wd.slice_off < 0 || wd.slice_len < 0 || wd.pad_left < 0 || wd.pad_right < 0 || wd.slice_off + wd.slice_len > genome->len ||
            lr > INT32_MAX)
            return fail(g_err, DSA_E_ARG, "window %lld lies outside the genome", (long long)k);
        if (wd.seq_len < 0 || wd.seq_off < 0 || wd.seq_off + wd.seq_len > pool_len)
            return fail(g_err, DSA_E_ARG, "sequence %lld lies outside the pool", (long long)k);
        tm.cells += (lr + 1) * ((int64_t)wd.seq_len + 1);
    }
    const uint8_t* d_genome = genome->bytes.p;
    const int rc = align_items(genome->device, match, mismatch, gap, pool, pool_len, windows, n_windows, min_score, scores, tm,
                               [d_genome](int items_per_lane, int n_waves, const uint8_t* d_pool, const la_window* d_wins, const Lane* d_lanes,
                                          const Wave* d_waves, uint32_t* d_ref, uint32_t* d_row) {
                                   if (items_per_lane == 2)
                                       hipLaunchKernelGGL(k_pack_win<2>, dim3(n_waves), dim3(256), 0, nullptr, d_genome, d_pool, d_wins, d_lanes,
                                                          d_waves, d_ref, d_row);
                                   else
                                       hipLaunchKernelGGL(k_pack_win<1>, dim3(n_waves), dim3(256), 0, nullptr, d_genome, d_pool, d_wins, d_lanes,
                                                          d_waves, d_ref, d_row);
                               });
    if (rc != DSA_OK) return rc;
    tm.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (timing) *timing = tm;
    return DSA_OK;
}

}  // extern "C"

// la_pairs.hpp.  The checks of la_align_windows_min, on pairs.
__attribute__((visibility("hidden"))) int la_align_pairs_device(int device, const uint8_t* d_bytes, int64_t bytes_len, int32_t match, int32_t mismatch,
                                                                int32_t gap, const la_pair* pairs, int64_t n_pairs, const int32_t* min_score,
                                                                int32_t* d_scores, la_timing* timing)
{
    const auto t_begin = std::chrono::steady_clock::now();
    la_timing tm{};
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !d_scores || !d_bytes))) return fail(g_err, DSA_E_ARG, "null argument");
    if (n_pairs >= (int64_t)1 << 31) return fail(g_err, DSA_E_LIMIT, "more than 2^31-1 pairs");
    for (int64_t k = 0; k < n_pairs; ++k) {
        const la_pair& pr = pairs[k];
        if (pr.ref_len < 0 || pr.seq_len < 0 || pr.ref_off < 0 || pr.seq_off < 0 || pr.ref_off + pr.ref_len > bytes_len || pr.seq_off + pr.seq_len > bytes_len)
            return fail(g_err, DSA_E_ARG, "pair %lld lies outside the bytes", (long long)k);
        tm.cells += ((int64_t)pr.ref_len + 1) * ((int64_t)pr.seq_len + 1);
    }
    const int rc = align_items(device, match, mismatch, gap, nullptr, 0, pairs, n_pairs, min_score, nullptr, tm,
                               [d_bytes](int items_per_lane, int n_waves, const uint8_t*, const la_pair* d_pairs, const Lane* d_lanes, const Wave* d_waves,
                                         uint32_t* d_ref, uint32_t* d_row) {
                                   if (items_per_lane == 2)
                                       hipLaunchKernelGGL(k_pack_pairs<2>, dim3(n_waves), dim3(256), 0, nullptr, d_bytes, d_pairs, d_lanes, d_waves, d_ref, d_row);
                                   else
                                       hipLaunchKernelGGL(k_pack_pairs<1>, dim3(n_waves), dim3(256), 0, nullptr, d_bytes, d_pairs, d_lanes, d_waves, d_ref, d_row);
                               },
                               d_scores);
    if (rc != DSA_OK) return rc;
    tm.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    if (timing) *timing = tm;
    return DSA_OK;
}
