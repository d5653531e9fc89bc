// eval_host — the host side of profiles/eval: the arithmetic of EvaluateGroup (tools_src/evaluate.hpp: std::map sums, the
// strict '>' walk, the kept list, the two serial sums) over a binary file of dsa_record, groups dealt to N threads.
//   g++ -std=c++17 -O2 -pthread -o profiles/microbench/eval_host profiles/microbench/eval_host.cpp
//   eval_host <records.bin> <threads> <repeats>      prints one line of milliseconds per repeat and a checksum
#include "../../include/defuse_dsa.h"
#include "../../tools_src/evaluate.hpp"

using namespace defuse;

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const size_t n = (size_t)std::ftell(f) / sizeof(dsa_record);
    std::fseek(f, 0, SEEK_SET);
    std::vector<dsa_record> rec(n);
    if (std::fread(rec.data(), sizeof(dsa_record), n, f) != n) return 2;
    std::fclose(f);
    const unsigned threads = (unsigned)std::atoi(argv[2]);
    std::vector<size_t> head;
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || rec[i].fusion_id != rec[i - 1].fusion_id) head.push_back(i);
    head.push_back(n);
    const size_t groups = head.size() - 1;
    for (int rep = 0; rep < std::atoi(argv[3]); ++rep) {
        std::vector<double> sum(threads, 0.0);
        std::vector<long long> kept_total(threads, 0);
        const auto t0 = std::chrono::steady_clock::now();
        run_threads(threads, [&](unsigned t) {
            std::map<std::pair<int, int>, int> splitScore;
            std::vector<size_t> kept;
            for (size_t g = groups * t / threads; g < groups * (t + 1) / threads; ++g) {
                splitScore.clear();
                for (size_t i = head[g]; i < head[g + 1]; ++i) splitScore[std::make_pair(rec[i].ref_first, rec[i].ref_second)] += rec[i].score;
                int maxScore = -1;
                std::pair<int, int> best;
                for (const auto& kv : splitScore)
                    if (kv.second > maxScore) { best = kv.first; maxScore = kv.second; }
                if (maxScore == -1) continue;
                kept.clear();
                for (size_t i = head[g]; i < head[g + 1]; ++i)
                    if (std::make_pair(rec[i].ref_first, rec[i].ref_second) == best) kept.push_back(i);
                double posSum = 0.0, minSum = 0.0;
                for (size_t i : kept) AddSplitStats(rec[i].read_first, rec[i].read_second, posSum, minSum);
                sum[t] += posSum + minSum;
                kept_total[t] += (long long)kept.size();
            }
        });
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        double s = 0;
        long long k = 0;
        for (unsigned t = 0; t < threads; ++t) { s += sum[t]; k += kept_total[t]; }
        std::printf("host_eval_ms %.3f threads %u groups %zu kept %lld checksum %.6f\n", ms, threads, groups, k, s);
    }
    return 0;
}
