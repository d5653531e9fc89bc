// tasktext_host.cpp — what a caller of task_store_create does on the host before it: the tool's own readers of the exon table
// and the regions file (tools_src/defuse_host.hpp), the three name maps, the resolution of every end and the packing into
// task_transcript[] / task_exon[] / task_pair[].  profiles/microbench/tasktext_throughput.py times it against taskt_*.
//
//   tasktext_host EXONS REGIONS NAMES REPEATS [PAIRS_OUT]
//
// NAMES: one sequence name per line, position = task_seq index = cand_region.ref.  Prints one line per repeat:
// "exons_ms X regions_ms Y pack_ms Z total_ms T"; with PAIRS_OUT the task_pair[] of the last repeat is written there.
// The readers are single-threaded (std::getline loops), so there is no thread count to vary.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/defuse_task.h"
#include "../../tools_src/defuse_host.hpp"

using Clock = std::chrono::steady_clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    std::unordered_map<std::string, int32_t> seq_index;
    {
        std::ifstream in(argv[3]);
        std::string line;
        while (std::getline(in, line)) seq_index.emplace(line, (int32_t)seq_index.size());
    }
    const int repeats = atoi(argv[4]);
    std::vector<task_pair> pairs;
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = Clock::now();
        defuse::ExonRegions E;
        {
            std::ifstream in(argv[1]);
            E.Read(in);
        }
        const auto t1 = Clock::now();
        const auto regions = defuse::ReadAlignRegionPairs(std::string(argv[2]));
        const auto t2 = Clock::now();
        // the exon table as task_exons_create takes it
        struct Row { std::string gene, chrom; int strand; const std::vector<defuse::Region>* exons; };
        std::unordered_map<std::string, Row> rows;
        std::vector<std::string> names;
        E.ForEachTranscript([&](const std::string& t, const std::string& gene, const std::string& chrom, int strand, const std::vector<defuse::Region>& ex) {
            names.push_back(t);
            rows.emplace(t, Row{gene, chrom, strand, &ex});
        });
        std::sort(names.begin(), names.end());
        std::unordered_map<std::string, int32_t> tindex, cindex;
        std::vector<task_transcript> tx;
        std::vector<task_exon> exons;
        std::vector<int32_t> chrom_ref;
        auto ref_of = [&](const std::string& n, int32_t absent) {
            auto it = seq_index.find(n);
            return it == seq_index.end() ? absent : it->second;
        };
        for (const std::string& t : names) {            // chromosomes by first appearance (the file's transcripts ascend)
            const std::string& chrom = rows.at(t).chrom;
            if (cindex.emplace(chrom, (int32_t)cindex.size()).second) chrom_ref.push_back(ref_of(chrom, (int32_t)(seq_index.size() + chrom_ref.size())));
        }
        for (const std::string& t : names) {
            const Row& r = rows.at(t);
            tindex.emplace(t, (int32_t)tx.size());
            tx.push_back(task_transcript{cindex.at(r.chrom), r.strand, (int32_t)exons.size(), (int32_t)r.exons->size(),
                                         ref_of(r.gene + "|" + t, (int32_t)(seq_index.size() + cindex.size() + tx.size()))});
            for (const auto& x : *r.exons) exons.push_back(task_exon{x.start, x.end});
        }
        // the pairs, resolved
        pairs.clear();
        pairs.reserve(regions.size());
        for (const auto& kv : regions) {
            task_pair p{};
            p.fusion_id = kv.first;
            for (int e = 0; e < 2; ++e) {
                const defuse::Location& l = kv.second[(size_t)e];
                std::string gene, transcript;
                int32_t t = -1;
                if (defuse::ParseTranscriptID(l.refName, gene, transcript)) {
                    auto it = tindex.find(transcript);
                    if (it != tindex.end()) t = it->second;
                }
                auto s = seq_index.find(l.refName);
                auto c = cindex.find(l.refName);
                p.end[e] = task_end{s == seq_index.end() ? -1 : s->second, t, c == cindex.end() ? -1 : c->second, l.strand, l.start, l.end};
            }
            pairs.push_back(p);
        }
        const auto t3 = Clock::now();
        printf("exons_ms %.3f regions_ms %.3f pack_ms %.3f total_ms %.3f transcripts %zu exons %zu pairs %zu\n", ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t0, t3), tx.size(),
               exons.size(), pairs.size());
    }
    if (argc > 5) {
        FILE* f = fopen(argv[5], "wb");
        if (!f || fwrite(pairs.data(), sizeof(task_pair), pairs.size(), f) != pairs.size()) return 1;
        fclose(f);
    }
    return 0;
}
