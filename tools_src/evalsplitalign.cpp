// evalsplitalign — drop-in replacement of the reference tool (tools/evalsplitalign.cpp:25-115):
// groups the fusion-id-sorted split alignments, picks the best supported breakpoint per fusion
// (SplitAlignmentTask::Evaluate, tools/SplitAlignment.cpp:484-594) and writes the .seq / .break /
// .predalign files (BreakPrediction::Write*, :596-624).  Host-only by default, like the reference: this stage has
// no DP and is I/O bound.  Ties between equally supported breakpoints go to the
// lexicographically smallest refSplit (canonical order of SURVEY.md 8(c)).
// DEFUSE_EVAL_GPU=1: the pieces only parse; the arithmetic of Evaluate for all groups is one call of the library
// (include/defuse_eval.h), and the three texts are formatted on the threads from its rows.
#include "../include/defuse_dsa.h"
#include "../include/defuse_eval.h"
#include "evaluate.hpp"
#include "task_cache.hpp"

using namespace defuse;

int main(int argc, char* argv[])
{
    CmdLine cmd("Fusion sequence prediction by split reads");
    cmd.add("f", "fasta", "Reference Fasta", "string");
    cmd.add("e", "exons", "Exon Regions Filename", "string");
    cmd.add("u", "ufrag", "Fragment Length Mean", "float");
    cmd.add("s", "sfrag", "Fragment Length Standard Deviation", "float");
    cmd.add("n", "minread", "Minimum Read Length", "integer");
    cmd.add("x", "maxread", "Maximum Read Length", "integer");
    cmd.add("r", "regions", "Fusion Regions Filename", "string");
    cmd.add("a", "align", "Split Alignments Filename", "string");
    cmd.add("q", "seq", "Sequences Filename", "string");
    cmd.add("b", "break", "Break Positions Filename", "string");
    cmd.add("p", "predalign", "Prediction Split Alignments Filename", "string");
    cmd.parse(argc, argv);

    // DEFUSE_DSA_TASK_CACHE=1: the tasks from "<regions>.dsatasks" when its key matches (task_cache.hpp)
    task_cache::SetUp cache;
    cache.on = task_cache::enabled();
    cache.timing = std::getenv("DEFUSE_TIMING") != nullptr;
    cache.tag = "[evalsplitalign]";
    cache.path = task_cache::path_for(cmd.str("regions"));
    const std::map<int, std::vector<Location>> regions = cache.read_regions(cmd.str("regions"), host_threads());
    std::map<int, SplitAlignmentTask> tasks = cache.tasks(cmd.str("fasta"), cmd.str("exons"), cmd.real("ufrag"), cmd.real("sfrag"),
                                                          cmd.integer("minread"), cmd.integer("maxread"), regions, host_threads(), nullptr);
    cache.keep(tasks, nullptr, host_threads());

    // DEFUSE_TIMING=1: the stages' wall times on stderr, one line at the end
    std::vector<std::pair<const char*, double>> stages;
    auto stageClock = std::chrono::steady_clock::now();
    auto stage = [&](const char* name) {
        const auto now = std::chrono::steady_clock::now();
        stages.emplace_back(name, std::chrono::duration<double, std::milli>(now - stageClock).count());
        stageClock = now;
    };
    auto report_stages = [&]() {
        if (!cache.timing) return;
        std::string line = "[evalsplitalign] stages (ms):";
        char buf[64];
        for (const auto& st : stages) line.append(buf, (size_t)snprintf(buf, sizeof buf, " %s %.1f", st.first, st.second));
        std::cerr << line << std::endl;
    };
    stage("setup");

    // The alignment file is mapped and cut into one piece per host thread at group boundaries (a group = a run of lines
    // with one fusion id, as ReadSortedAlignments forms them); the pieces are evaluated side by side and their three texts
    // written in order.  A malformed line ends the run as in the reference: everything before it is written, then the
    // message.
    MappedText text;
    text.load(cmd.str("align"), "Error: Unable to open ");
    OrderedFileWriter seqFile, breakFile, predFile;
    if (!seqFile.open_file(cmd.str("seq"))) die("Error: Unable to open " + cmd.str("seq"));
    if (!breakFile.open_file(cmd.str("break"))) die("Error: Unable to open " + cmd.str("break"));
    if (!predFile.open_file(cmd.str("predalign"))) die("Error: Unable to open " + cmd.str("predalign"));
    const SplitAlignmentTask emptyTask;                  // operator[] of the reference: an unknown id evaluates against an empty task

    unsigned nPieces = host_threads();
    if (text.size() < ((size_t)1 << 20) && !std::getenv("DEFUSE_THREADS")) nPieces = 1;
    auto first_field = [&](size_t pos, size_t& n) {       // the fusion id column of the line at pos, as text
        const size_t e = text.line_end(pos);
        const char* tab = (const char*)memchr(text.data() + pos, '\t', e - pos);
        n = tab ? (size_t)(tab - (text.data() + pos)) : e - pos - ((e > pos && text[e - 1] == '\n') ? 1 : 0);
        return text.data() + pos;
    };
    std::vector<size_t> cut = text.cut_lines(0, text.size(), nPieces);
    for (unsigned t = 1; t < nPieces; ++t) {              // move every cut forward to the next change of the fusion id column
        size_t pos = std::max(cut[t], cut[t - 1]);
        while (pos > 0 && pos < text.size()) {
            size_t prev = pos - 1;                        // start of the previous line
            while (prev > 0 && text[prev - 1] != '\n') --prev;
            size_t na, nb;
            const char* a = first_field(prev, na);
            const char* b = first_field(pos, nb);
            int ia, ib;                                       // compared as the integers the reader casts them to ("013" continues group 13)
            if (!field_int(a, na, ia) || !field_int(b, nb, ib) || ia != ib) break;
            pos = text.line_end(pos);
        }
        cut[t] = pos;
    }
    const char* gpuEnv = std::getenv("DEFUSE_EVAL_GPU");
    const bool onGpu = gpuEnv && gpuEnv[0] && std::strcmp(gpuEnv, "0") != 0;
    struct Piece {
        std::string seq, brk, pred, error;
        std::vector<dsa_record> records;                    // DEFUSE_EVAL_GPU: the groups a sequential reader would have evaluated,
        std::vector<size_t> group_start;                    // as records, and where each begins
        size_t last_seq = 0, last_brk = 0, last_pred = 0;   // where the texts of the piece's last group begin
        bool cancels_previous = false;                      // its FIRST line is malformed in a way that ends the run inside the previous group's look-ahead
        bool empty = true;
    };
    std::vector<Piece> pieces(nPieces);
    run_threads(nPieces, [&](unsigned t) {
        Piece& out = pieces[t];
        std::vector<SplitAlignment> alignments;
        std::vector<const SplitAlignment*> kept;
        std::map<std::pair<int, int>, int> splitScore;
        SplitAlignment pending;
        EvalTexts texts;
        auto evaluate = [&]() {
            if (onGpu) {
                out.group_start.push_back(out.records.size());
                for (const SplitAlignment& a : alignments)
                    out.records.push_back(dsa_record{a.fusionID, a.fragmentIndex, a.readEnd, a.revComp, a.refSplit.first, a.refSplit.second,
                                                     a.readSplit.first, a.readSplit.second, a.score, 0});
                alignments.clear();
                return;
            }
            out.last_seq = out.seq.size(); out.last_brk = out.brk.size(); out.last_pred = out.pred.size();
            auto ti = tasks.find(alignments.front().fusionID);
            const SplitAlignmentTask& task = ti == tasks.end() ? emptyTask : ti->second;
            texts.seq.clear(); texts.brk.clear(); texts.pred.clear();
            EvaluateGroup(task, alignments, texts, kept, splitScore);
            out.seq += texts.seq; out.brk += texts.brk; out.pred += texts.pred;
            alignments.clear();
        };
        for (size_t pos = cut[t]; pos < cut[t + 1];) {
            const size_t e = text.line_end(pos);
            const size_t len = (e > pos && text[e - 1] == '\n') ? e - 1 - pos : e - pos;
            bool id_read = false;
            out.error = parse_line(text.data() + pos, len, pending, id_read);
            pos = e;
            const bool first_line = out.empty;
            out.empty = false;
            if (!out.error.empty()) {
                if (first_line && !id_read) out.cancels_previous = true;
                // the reference reads one line ahead: a malformed line that at least opens a new group (seven fields, a
                // readable id different from the running group's) lets the running group through first; any other malformed
                // line ends the run inside the reader, before the running group is evaluated
                if (!(id_read && !alignments.empty() && pending.fusionID != alignments.front().fusionID)) alignments.clear();
                break;
            }
            if (!alignments.empty() && pending.fusionID != alignments.front().fusionID) evaluate();
            alignments.push_back(pending);
        }
        if (!alignments.empty()) evaluate();
    });
    stage(onGpu ? "parse" : "parse+evaluate");
    if (onGpu) {
        // All records a sequential reader would have evaluated, in order: the pieces up to the first with a malformed line,
        // without the last group of a piece that the next piece's first line cancels.
        std::vector<dsa_record> records;
        std::vector<size_t> groupStart;
        std::string error;
        for (unsigned t = 0; t < nPieces; ++t) {
            Piece& pc = pieces[t];
            size_t nGroups = pc.group_start.size(), nRecords = pc.records.size();
            for (unsigned u = t + 1; u < nPieces; ++u) {
                if (pieces[u].empty) continue;
                if (pieces[u].cancels_previous && nGroups) nRecords = pc.group_start[--nGroups];
                break;
            }
            for (size_t k = 0; k < nGroups; ++k) groupStart.push_back(records.size() + pc.group_start[k]);
            records.insert(records.end(), pc.records.begin(), pc.records.begin() + (std::ptrdiff_t)nRecords);
            std::vector<dsa_record>().swap(pc.records);
            if (!pc.error.empty()) { error = pc.error; break; }
        }
        const size_t nGroups = groupStart.size();
        groupStart.push_back(records.size());
        std::vector<eval_group> rows(nGroups);
        std::vector<int64_t> keptList(records.size());
        if (!records.empty()) {                              // no lines to evaluate: no device
            eval_ctx* ctx = nullptr;
            int64_t gotGroups = 0, gotKept = 0;
            if (eval_create(dsa_pick_device(), &ctx) != 0) die(std::string("Error: GPU evaluation failed: ") + eval_last_error());
            if (eval_groups(ctx, records.data(), (int64_t)records.size(), rows.data(), (int64_t)nGroups, &gotGroups, keptList.data(),
                            (int64_t)keptList.size(), &gotKept) != 0)
                die(std::string("Error: GPU evaluation failed: ") + eval_last_error());
            if (cache.timing) {
                eval_timing tm;
                eval_get_timing(ctx, &tm);
                std::fprintf(stderr, "[evalsplitalign] eval gpu: upload %.3f ms, kernels %.3f ms, download %.3f ms; %lld records, %lld groups, %lld splits, %lld kept, %lld flagged\n",
                             tm.upload_ms, tm.device_ms, tm.download_ms, (long long)tm.n_records, (long long)tm.n_groups, (long long)tm.n_runs,
                             (long long)tm.n_kept, (long long)tm.n_flagged);
            }
            eval_destroy(ctx);
            // the library forms groups from runs of equal ids; they must be the parser's
            bool same = (size_t)gotGroups == nGroups;
            for (size_t k = 0; same && k < nGroups; ++k)
                same = (size_t)rows[k].first_record == groupStart[k] && (size_t)rows[k].n_records == groupStart[k + 1] - groupStart[k];
            if (!same) die("Error: GPU evaluation failed: its groups are not the reader's");
        }
        stage("gpu");
        // the texts, one share of the groups (by records) per thread, written in order
        std::vector<size_t> share(nPieces + 1, nGroups);
        share[0] = 0;
        for (unsigned t = 1; t < nPieces; ++t) {
            const size_t want = records.size() / nPieces * t;
            share[t] = (size_t)(std::lower_bound(groupStart.begin(), groupStart.begin() + (std::ptrdiff_t)nGroups, want) - groupStart.begin());
        }
        run_threads(nPieces, [&](unsigned t) {
            Piece& out = pieces[t];
            EvalTexts texts;
            for (size_t k = share[t]; k < share[t + 1]; ++k) {
                const eval_group& row = rows[k];
                auto ti = tasks.find(row.fusion_id);
                const SplitAlignmentTask& task = ti == tasks.end() ? emptyTask : ti->second;
                GroupVerdict v;
                const int64_t* kp = keptList.data() + row.kept_off;
                if (!(row.status & EVAL_NO_SPLIT)) {
                    v.found = true;
                    v.best = std::make_pair(row.best_first, row.best_second);
                    v.count = (int)row.count;
                    v.posSum = row.pos_sum; v.minSum = row.min_sum;
                    if (row.status & EVAL_HOST_STATS) {       // a zero range among the kept: the host's own NaN and infinities
                        v.posSum = v.minSum = 0.0;
                        for (int64_t j = 0; j < row.count; ++j) AddSplitStats(records[(size_t)kp[j]].read_first, records[(size_t)kp[j]].read_second, v.posSum, v.minSum);
                    }
                }
                texts.seq.clear(); texts.brk.clear(); texts.pred.clear();
                WriteVerdict(task, row.fusion_id, v, texts);
                out.seq += texts.seq; out.brk += texts.brk;
                for (int64_t j = 0; v.found && j < row.count; ++j) {
                    const dsa_record& r = records[(size_t)kp[j]];
                    SplitAlignment a;
                    a.fusionID = r.fusion_id; a.fragmentIndex = r.frag; a.readEnd = r.read_end; a.revComp = r.revcomp;
                    a.refSplit = std::make_pair(r.ref_first, r.ref_second);
                    a.readSplit = std::make_pair(r.read_first, r.read_second);
                    a.score = r.score;
                    a.Write(out.pred);
                }
            }
        });
        stage("format");
        for (unsigned t = 0; t < nPieces; ++t) {
            seqFile.write_round({pieces[t].seq}, 1);
            breakFile.write_round({pieces[t].brk}, 1);
            predFile.write_round({pieces[t].pred}, 1);
        }
        if (!error.empty()) {
            seqFile.close_file(); breakFile.close_file(); predFile.close_file();
            die(error);
        }
        if (!seqFile.close_file() || !breakFile.close_file() || !predFile.close_file()) die("Error: failed writing the predictions");
        stage("write");
        report_stages();
        return 0;
    }
    for (unsigned t = 0; t < nPieces; ++t) {
        for (unsigned u = t + 1; u < nPieces; ++u) {          // the next piece that holds lines
            if (pieces[u].empty) continue;
            if (pieces[u].cancels_previous) {                 // a sequential reader meets that line while it still collects this piece's last group
                pieces[t].seq.resize(pieces[t].last_seq); pieces[t].brk.resize(pieces[t].last_brk); pieces[t].pred.resize(pieces[t].last_pred);
            }
            break;
        }
        seqFile.write_round({pieces[t].seq}, 1);
        breakFile.write_round({pieces[t].brk}, 1);
        predFile.write_round({pieces[t].pred}, 1);
        if (!pieces[t].error.empty()) {
            seqFile.close_file(); breakFile.close_file(); predFile.close_file();
            die(pieces[t].error);
        }
    }
    if (!seqFile.close_file() || !breakFile.close_file() || !predFile.close_file()) die("Error: failed writing the predictions");
    stage("write");
    report_stages();
    return 0;
}
