// task_host — the host side of profiles/task: what a caller of the resident chain does today before its first call, with the
// tool's own CreateTasks (tools_src/defuse_host.hpp: FastaIndex over the mapped FASTA, ExonRegions, SplitAlignmentTask::
// Initialize on N threads), then the packing of its result and bat_windows_create + pred_tasks_create of it.
//   g++ -std=c++17 -O2 -pthread -o profiles/microbench/task_host profiles/microbench/task_host.cpp defuse_amd/libdefuse_dsa.so \
//       -Wl,-rpath,$PWD/defuse_amd
//   task_host <ref.fa> <exons.txt> <regions.txt> <mean> <sd> <minread> <maxread> <threads> <repeats> [dump prefix]
// One line of milliseconds per repeat.  With a dump prefix the tasks of the last repeat are written for the comparison with the
// device path: <prefix>.rec (per task in ascending fusion id 11 int32: id, seq_start[2], seq_len[2], seq_strand[2], remainder
// lengths[2], regions[2]), <prefix>.win, <prefix>.rem (the bytes back to back), <prefix>.reg (a text line per mate region).
#include "../../include/defuse_bat.h"
#include "../../include/defuse_pred.h"
#include "../../tools_src/defuse_host.hpp"

using namespace defuse;

static void dump(const std::string& path, const void* p, size_t n)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) die("cannot write " + path);
    std::fclose(f);
}

int main(int argc, char** argv)
{
    if (argc < 10) return 2;
    const std::string fasta = argv[1], exons = argv[2], regions_file = argv[3];
    const double mean = std::atof(argv[4]), sd = std::atof(argv[5]);
    const int min_read = std::atoi(argv[6]), max_read = std::atoi(argv[7]);
    const unsigned threads = (unsigned)std::atoi(argv[8]);
    const int repeats = std::atoi(argv[9]);
    const std::string prefix = argc > 10 ? argv[10] : "";
    const std::map<int, std::vector<Location>> regions = ReadAlignRegionPairs(regions_file);
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    // (the device is up before anything is timed: a chain caller's is)
    bat_batch* warm = nullptr;
    if (bat_batch_create(0, &warm) != DSA_OK) die(std::string("Error: ") + bat_last_error());
    for (int rep = 0; rep < repeats; ++rep) {
        const auto t0 = now();
        const std::map<int, SplitAlignmentTask> tasks = CreateTasks(fasta, exons, mean, sd, min_read, max_read, regions, threads);
        const auto t1 = now();
        std::vector<dsa_fusion> wfus;
        std::vector<pred_task> ptask;
        std::vector<uint8_t> wbytes, rbytes;
        wfus.reserve(tasks.size());
        ptask.reserve(tasks.size());
        size_t wtotal = 0, rtotal = 0;
        for (const auto& kv : tasks)
            for (int e = 0; e < 2; ++e) {
                wtotal += kv.second.mSplitAlignSeq[e].size();
                rtotal += kv.second.mSplitRemainderSeq[e].size();
            }
        wbytes.resize(wtotal);
        rbytes.resize(rtotal);
        size_t wo = 0, ro = 0;
        for (const auto& kv : tasks) {
            const SplitAlignmentTask& t = kv.second;
            dsa_fusion f{t.mFusionID, 0, 0, 0, 0};
            pred_task p{};
            p.fusion_id = t.mFusionID;
            for (int e = 0; e < 2; ++e) {
                const size_t wn = t.mSplitAlignSeq[e].size(), rn = t.mSplitRemainderSeq[e].size();
                (e == 0 ? f.ref0_off : f.ref1_off) = (int32_t)wo;
                (e == 0 ? f.ref0_len : f.ref1_len) = (int32_t)wn;
                if (wn) std::memcpy(&wbytes[wo], t.mSplitAlignSeq[e].data(), wn);
                if (rn) std::memcpy(&rbytes[ro], t.mSplitRemainderSeq[e].data(), rn);
                p.seq_start[e] = t.mSplitAlignSeqStart[e];
                p.seq_len[e] = t.mSplitAlignSeqLength[e];
                p.seq_strand[e] = t.mSplitSeqStrand[e];
                p.rem_off[e] = (int64_t)ro;
                p.rem_len[e] = (int32_t)rn;
                wo += wn;
                ro += rn;
            }
            wfus.push_back(f);
            ptask.push_back(p);
        }
        const auto t2 = now();
        bat_windows* windows = nullptr;
        pred_tasks* ptasks = nullptr;
        if (bat_windows_create(0, wbytes.data(), (int64_t)wbytes.size(), wfus.data(), (int32_t)wfus.size(), &windows) != DSA_OK)
            die(std::string("Error: ") + bat_last_error());
        const auto t3 = now();
        if (pred_tasks_create(0, windows, rbytes.data(), (int64_t)rbytes.size(), ptask.data(), (int64_t)ptask.size(), &ptasks) != DSA_OK)
            die(std::string("Error: ") + pred_last_error());
        const auto t4 = now();
        std::printf("host_task threads %u create_tasks_ms %.3f pack_ms %.3f windows_create_ms %.3f pred_tasks_create_ms %.3f total_ms %.3f tasks %zu "
                    "window_bytes %zu rem_bytes %zu\n", threads, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t0, t4), tasks.size(), wbytes.size(),
                    rbytes.size());
        std::fflush(stdout);
        pred_tasks_destroy(ptasks);
        bat_windows_destroy(windows);
        if (rep + 1 == repeats && !prefix.empty()) {
            std::vector<int32_t> rec;
            std::string reg;
            for (const auto& kv : tasks) {
                const SplitAlignmentTask& t = kv.second;
                const int32_t row[11] = {t.mFusionID, t.mSplitAlignSeqStart[0], t.mSplitAlignSeqStart[1], t.mSplitAlignSeqLength[0], t.mSplitAlignSeqLength[1],
                                         t.mSplitSeqStrand[0], t.mSplitSeqStrand[1], (int32_t)t.mSplitRemainderSeq[0].size(), (int32_t)t.mSplitRemainderSeq[1].size(),
                                         (int32_t)t.mMateRegions[0].size(), (int32_t)t.mMateRegions[1].size()};
                rec.insert(rec.end(), row, row + 11);
                for (int e = 0; e < 2; ++e)
                    for (const Location& m : t.mMateRegions[e])
                        reg += m.refName + "\t" + std::to_string(m.strand) + "\t" + std::to_string(m.start) + "\t" + std::to_string(m.end) + "\n";
            }
            dump(prefix + ".rec", rec.data(), rec.size() * sizeof(int32_t));
            dump(prefix + ".win", wbytes.data(), wbytes.size());
            dump(prefix + ".rem", rbytes.data(), rbytes.size());
            dump(prefix + ".reg", reg.data(), reg.size());
        }
    }
    bat_batch_destroy(warm);
    return 0;
}
