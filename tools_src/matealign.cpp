// matealign — drop-in replacement of the reference's mate rescue tool (tools/matealign.cpp:39-205): same command line
// (-m match, -x mismatch, -g gap, optional -t threshold, -s search length, -r reference FASTA, -1 / -2 FASTQ files),
// SAM alignments on stdin, stdout lines `fragment \t score \t percent`.  Every read is aligned (SimpleAligner::Align,
// tools/SimpleAligner.cpp:24-64) against a window of the genome next to each alignment of its mate.  The genome is uploaded
// once; the device cuts the windows out of it (la_align_windows_min, include/defuse_la.h), so only the reads and a 40-byte
// descriptor per pair cross the bus.  There is no CPU fallback: without a HIP device the tool exits 1.
//
// One deviation: where the reference ends in an uncaught exception (a read fragment that is not an integer, a window that
// starts beyond its contig), this tool prints an `Error:` line and exits 1.
#include "../include/defuse_dsa.h"
#include "../include/defuse_la.h"
#include "defuse_host.hpp"

using namespace defuse;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct MateAlignment {          // CompactPosition of the reference, keyed by the ReadID of the aligned read
    int key;                    // pack_id(fragment, read end)
    int name;                   // index into the reference names of the SAM input
    int strand;
    int position;               // pos on the plus strand, pos + len(SEQ) - 1 on the minus strand
};

struct Contig { int64_t off; int len; };

struct Scorer {
    int matchScore, misMatchScore, gapScore;
    double threshold;
    const std::vector<uint8_t>* genome = nullptr;
    la_genome* dev_genome = nullptr;
    double t_upload = 0, t_device = 0, t_output = 0;
    int64_t n_pairs = 0, n_batches = 0;
    // the batch: reads in a pool, one window per (read, mate alignment) in output order
    std::vector<uint8_t> pool;
    std::vector<la_window> windows;
    std::vector<uint32_t> frags;        // what the line prints: ReadID::fragmentIndex, the low 31 bits
    std::vector<int32_t> max_scores, need;

    size_t bytes() const { return pool.size() + windows.size() * (sizeof(la_window) + 12); }

    // scores the batch and writes its lines (the reference prints every line as it goes, so a later error still leaves the
    // earlier lines on stdout)
    void flush()
    {
        if (windows.empty()) return;
        double t = now();
        if (!dev_genome) {              // the device is opened with the first batch: input errors before it need no GPU
            const int device = dsa_pick_device();         // as the other tools: DEFUSE_GPU, else pid mod device count
            if (la_genome_create(device, genome->data(), (int64_t)genome->size(), &dev_genome) != 0)
                die(std::string("Error: GPU genome upload failed: ") + la_last_error());
            t_upload = now() - t;
            t = now();
        }
        std::vector<int32_t> scores(windows.size());
        if (la_align_windows_min(dev_genome, matchScore, misMatchScore, gapScore, pool.data(), (int64_t)pool.size(), windows.data(),
                                 (int64_t)windows.size(), need.data(), scores.data(), nullptr) != 0)
            die(std::string("Error: GPU alignment failed: ") + la_last_error());
        t_device += now() - t;
        t = now();
        std::string out;
        char id[16];
        for (size_t k = 0; k < windows.size(); ++k) {
            const char* e = put_int(id, (int)frags[k]);
            append_score_line(out, std::string_view(id, (size_t)(e - id)), scores[k], max_scores[k], threshold);  // tools/matealign.cpp:191-203
            if (out.size() > (1u << 22)) { fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
        }
        fwrite(out.data(), 1, out.size(), stdout);
        fflush(stdout);
        t_output += now() - t;
        n_pairs += (int64_t)windows.size();
        ++n_batches;
        pool.clear();
        windows.clear();
        frags.clear();
        max_scores.clear();
        need.clear();
    }
    [[noreturn]] void fail(const std::string& msg)
    {
        flush();
        die(msg);
    }
};

}  // namespace

int main(int argc, char* argv[])
{
    CmdLine cmd("Mate Realignment Tool");
    cmd.add("m", "match", "Match Score", "int");
    cmd.add("x", "mismatch", "Mismatch Score", "int");
    cmd.add("g", "gap", "Gap Score", "int");
    cmd.add_optional("t", "threshold", "Percent Perfect Threshold", "float", "0");
    cmd.add("s", "searchlength", "Search Length", "integer");
    cmd.add("r", "reference", "Reference Sequences Fasta", "string");
    cmd.add("1", "seq1", "End 1 Sequences", "string");
    cmd.add("2", "seq2", "End 2 Sequences", "string");
    cmd.parse(argc, argv);
    const int searchLength = cmd.integer("searchlength");

    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    double t_stage = now();
    auto stage = [&](const char* name) {
        const double t = now();
        if (timing) std::cerr << "[matealign] " << name << " " << (t - t_stage) << " s" << std::endl;
        t_stage = t;
    };

    // ---- SAM on stdin (tools/matealign.cpp:78-158) ----
    std::vector<MateAlignment> alignments;
    std::vector<std::string> names;                       // NameIndex: reference names in order of first use
    std::unordered_map<std::string, int> name_index;
    {
        LineReader reader(stdin);
        const char* line;
        size_t len;
        size_t lineNumber = 0;
        int read_end = 0;
        while (reader.next(line, len)) {
            lineNumber++;
            SamFields a;
            const int kind = ParseSamLine(line, len, a, read_end);
            if (kind == 1) continue;                              // header line, rname "*"
            if (kind >= 2) DieSamLine(kind, lineNumber);
            if (a.fragment[a.fragment_len] != '/') DieSamLine(5, lineNumber);     // the qname must be exactly "x/1" or "x/2"
            int frag;
            if (!field_int(a.fragment, a.fragment_len, frag)) DieSamLine(4, lineNumber);
            std::string rname(a.reference, a.reference_len);
            auto it = name_index.find(rname);
            if (it == name_index.end()) {
                it = name_index.emplace(rname, (int)names.size()).first;
                names.push_back(rname);
            }
            alignments.push_back({pack_id(frag, read_end), it->second, a.strand, a.strand == PlusStrand ? a.region.start : a.region.end});
        }
    }
    std::stable_sort(alignments.begin(), alignments.end(), [](const MateAlignment& x, const MateAlignment& y) { return x.key < y.key; });
    std::cerr << "Read alignments" << std::endl;
    stage("sam");

    // ---- FASTA (Sequences::Read, tools/Sequences.cpp:18-57): the whole header line names a contig, the last one of a name wins ----
    std::vector<uint8_t> genome;
    std::unordered_map<std::string, Contig> contigs;
    {
        const std::string fasta = cmd.str("reference");
        FILE* f = fopen(fasta.c_str(), "rb");
        if (!f) die("Error: unable to open file " + fasta);
        LineReader reader(f);
        const char* line;
        size_t len;
        std::string id;
        size_t begin = 0;
        auto finish = [&]() {
            if (!id.empty()) contigs[id] = Contig{(int64_t)begin, (int)(genome.size() - begin)};
            else genome.resize(begin);                          // sequence without a name: dropped
        };
        while (reader.next(line, len)) {
            if (len == 0) continue;
            if (line[0] == '>') {
                finish();
                id.assign(line + 1, len - 1);
                begin = genome.size();
            } else {
                genome.insert(genome.end(), (const uint8_t*)line, (const uint8_t*)line + len);
            }
        }
        finish();
        fclose(f);
    }
    std::cerr << "Read reference fasta" << std::endl;
    stage("fasta");

    // ---- reads (IReadStream::Create for both files, then every record of file 1, then of file 2) ----
    FastqReader reads[2];
    const bool ok1 = reads[0].open(cmd.str("seq1"), std::cerr);
    const bool ok2 = reads[1].open(cmd.str("seq2"), std::cerr);
    if (!ok1 || !ok2) {
        std::cout << "Error: unable to read sequences" << std::endl;
        return 1;
    }
    std::vector<int> name_contig(names.size(), -1);       // index into contig_list, -1: not in the FASTA
    std::vector<Contig> contig_list;
    for (size_t k = 0; k < names.size(); ++k) {
        auto it = contigs.find(names[k]);
        if (it != contigs.end()) {
            name_contig[k] = (int)contig_list.size();
            contig_list.push_back(it->second);
        }
    }

    Scorer sc;
    sc.matchScore = cmd.integer("match");
    sc.misMatchScore = cmd.integer("mismatch");
    sc.gapScore = cmd.integer("gap");
    sc.threshold = cmd.real("threshold");
    sc.genome = &genome;
    const size_t flush_bytes = (size_t)1 << 30;           // bounds host and device memory on very large inputs
    double t_reads = 0;
    double t_mark = now();
    FastqRecord rec;
    for (int file = 0; file < 2; ++file) {
        while (reads[file].next(rec, std::cerr)) {
            int frag;
            if (!field_int(rec.fragment.data(), rec.fragment.size(), frag)) {      // reference: uncaught bad_lexical_cast
                t_reads += now() - t_mark;
                sc.fail("Error: bad integer '" + std::string(rec.fragment) + "' in read name " + rec.name);
            }
            const int other = pack_id(frag, 1 - rec.end);
            auto lo = std::lower_bound(alignments.begin(), alignments.end(), other, [](const MateAlignment& x, int k) { return x.key < k; });
            if (lo == alignments.end() || lo->key != other) continue;
            if (rec.sequence.size() > (size_t)INT32_MAX) sc.fail("Error: read longer than 2^31-1 bases: " + rec.name);
            const int64_t seq_off = (int64_t)sc.pool.size();
            const int seq_len = (int)rec.sequence.size();
            sc.pool.insert(sc.pool.end(), rec.sequence.begin(), rec.sequence.end());
            const int maxScore = score_max(rec.sequence.size(), sc.matchScore);
            const int32_t need = threshold_min_score(maxScore, sc.threshold);
            for (auto it = lo; it != alignments.end() && it->key == other; ++it) {
                const int ci = name_contig[(size_t)it->name];
                if (ci < 0) {
                    t_reads += now() - t_mark;
                    sc.fail("Error: Unable to find sequence " + names[(size_t)it->name]);     // Sequences::Get, tools/Sequences.cpp:62-66
                }
                // tools/matealign.cpp:180-189: [pos, pos + s] reverse-complemented for a plus-strand mate, [anchor - s, anchor] else
                const bool plus = it->strand == PlusStrand;
                const int start = (int)(plus ? (int64_t)it->position : (int64_t)it->position - searchLength);
                const int end = (int)(plus ? (int64_t)it->position + searchLength : (int64_t)it->position);
                // Sequences::Get (tools/Sequences.cpp:68-78) with its int arithmetic
                const Contig& c = contig_list[(size_t)ci];
                const int seqStart = std::max(1, start);
                const int prependN = seqStart - start;
                const int seqEnd = std::min(c.len, end);
                const int appendN = end - seqEnd;
                const int seqLength = seqEnd - seqStart + 1;
                if (seqStart - 1 > c.len) {                       // reference: substr throws std::out_of_range, uncaught
                    t_reads += now() - t_mark;
                    sc.fail("Error: window start " + std::to_string(start) + " lies beyond the end of sequence " + names[(size_t)it->name] +
                            " (length " + std::to_string(c.len) + ")");
                }
                la_window w{};
                w.slice_off = c.off + seqStart - 1;
                w.slice_len = seqLength >= 0 ? seqLength : c.len - (seqStart - 1);      // a negative length takes the contig's tail
                w.pad_left = prependN;
                w.pad_right = appendN;
                w.seq_off = seq_off;
                w.seq_len = seq_len;
                w.revcomp = plus ? 1 : 0;
                sc.windows.push_back(w);
                sc.frags.push_back((uint32_t)frag & 0x7FFFFFFFu);
                sc.max_scores.push_back(maxScore);
                sc.need.push_back(need);
            }
            if (sc.bytes() >= flush_bytes) {
                t_reads += now() - t_mark;
                sc.flush();
                t_mark = now();
            }
        }
    }
    t_reads += now() - t_mark;
    sc.flush();
    if (timing) {
        std::cerr << "[matealign] reads " << t_reads << " s" << std::endl;
        std::cerr << "[matealign] genome upload " << sc.t_upload << " s (" << genome.size() << " bytes)" << std::endl;
        std::cerr << "[matealign] device " << sc.t_device << " s (" << sc.n_pairs << " pairs, " << sc.n_batches << " batches)" << std::endl;
        std::cerr << "[matealign] output " << sc.t_output << " s" << std::endl;
    }
    la_genome_destroy(sc.dev_genome);
    return 0;
}
