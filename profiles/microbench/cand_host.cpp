// cand_host — the host side of profiles/cand: what dosplitalign's host stage does between the SAM records and the candidates,
// with the tool's own classes (tools_src/defuse_host.hpp: BinnedLocations, FlatSet64, run_threads) on binary files of
// cand_region / cand_alignment: Add + Finish, Overlapping per alignment on N threads (pieces of the alignments), the
// de-duplication with the keys dealt to the threads by hash, and the count of the kept candidates.  No text is parsed.
//   g++ -std=c++17 -O2 -pthread -o profiles/microbench/cand_host profiles/microbench/cand_host.cpp
//   cand_host <regions.bin> <alignments.bin> <threads> <repeats>     one line of milliseconds per repeat
#include "../../include/defuse_cand.h"
#include "../../tools_src/defuse_host.hpp"

using namespace defuse;

template <typename T>
static std::vector<T> slurp(const char* path)
{
    std::vector<T> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    std::fseek(f, 0, SEEK_END);
    v.resize((size_t)std::ftell(f) / sizeof(T));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
    std::fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const std::vector<cand_region> regs = slurp<cand_region>(argv[1]);
    const std::vector<cand_alignment> als = slurp<cand_alignment>(argv[2]);
    const unsigned threads = (unsigned)std::atoi(argv[3]);
    if (regs.empty() || als.empty() || !threads) return 2;
    int n_refs = 0;
    for (const cand_region& g : regs) n_refs = std::max(n_refs, g.ref + 1);
    for (const cand_alignment& a : als) n_refs = std::max(n_refs, a.ref + 1);
    std::vector<std::string> name((size_t)n_refs);
    for (int r = 0; r < n_refs; ++r) name[(size_t)r] = "ref" + std::to_string(r);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    for (int rep = 0; rep < std::atoi(argv[4]); ++rep) {
        const auto t0 = now();
        BinnedLocations binned(CAND_BIN_SPACING);
        for (const cand_region& g : regs) {
            Location loc;
            loc.refName = name[(size_t)g.ref];
            loc.strand = g.strand;
            loc.start = g.start;
            loc.end = g.end;
            binned.Add(g.id, loc);
        }
        binned.Finish();
        const auto t1 = now();
        struct Piece { std::vector<int> ids; std::vector<uint32_t> first; std::vector<uint8_t> keep; };
        std::vector<Piece> pieces(threads);
        run_threads(threads, [&](unsigned t) {
            Piece& pc = pieces[t];
            std::vector<int> overlapping;
            const size_t lo = als.size() * t / threads, hi = als.size() * (t + 1) / threads;
            for (size_t k = lo; k < hi; ++k) {
                const cand_alignment& a = als[k];
                pc.first.push_back((uint32_t)pc.ids.size());
                if (a.ref < 0) continue;
                binned.Overlapping(name[(size_t)a.ref], a.strand, Region{a.start, a.end}, overlapping);
                pc.ids.insert(pc.ids.end(), overlapping.begin(), overlapping.end());
            }
            pc.first.push_back((uint32_t)pc.ids.size());
            pc.keep.assign(pc.ids.size(), 0);
        });
        const auto t2 = now();
        size_t visited = 0;
        for (const Piece& pc : pieces) visited += pc.ids.size();
        std::vector<FlatSet64> seen(threads, FlatSet64(1 << 12));
        run_threads(threads, [&](unsigned t) {
            FlatSet64& mine = seen[t];
            mine.reserve(visited / threads + visited / (4 * threads) + 64);
            for (unsigned p = 0; p < threads; ++p) {
                Piece& pc = pieces[p];
                const size_t lo = als.size() * p / threads;
                for (size_t k = 0; k + 1 < pc.first.size(); ++k) {
                    const cand_alignment& a = als[lo + k];
                    for (uint32_t x = pc.first[k]; x < pc.first[k + 1]; ++x) {
                        const int cid = pc.ids[x];
                        const uint64_t key = ((uint64_t)(uint32_t)(cid & 0x7FFFFFFF) << 33) | ((uint64_t)(uint32_t)a.fragment << 2) |
                                             ((uint64_t)(a.read_end == 0 ? 1 : 0) << 1) | (uint64_t)(cid < 0 ? 0 : 1);
                        if (FlatSet64::hash(key ^ 0x9e3779b97f4a7c15ULL) % threads != t) continue;
                        if (mine.insert(key)) pc.keep[x] = 1;
                    }
                }
            }
        });
        size_t kept = 0;
        for (const Piece& pc : pieces)
            for (uint8_t k : pc.keep) kept += k;
        const auto t3 = now();
        std::printf("host_cand threads %u table_ms %.3f overlap_ms %.3f dedup_ms %.3f enumerate_ms %.3f visited %zu kept %zu\n", threads, ms(t0, t1),
                    ms(t1, t2), ms(t2, t3), ms(t1, t3), visited, kept);
    }
    return 0;
}
