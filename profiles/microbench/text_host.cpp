// The tools' host parsers over text that profiles/microbench/text_throughput.py has cut at line (FASTQ: record) starts, one
// thread per piece: LineReader + ParseSamLine + field_int of the fragment + the name lookup for SAM, FastqReader::next +
// field_int + ReadStore::put (AddReads) for FASTQ.
//
//     g++ -std=c++17 -O2 -pthread -o profiles/microbench/text_host profiles/microbench/text_host.cpp
//     text_host sam|fastq <repeats> <piece> [<piece> ...]
//
// Prints per repeat "<mode> threads <n> ms <wall> records <n> check <sum>".  The clock is steady_clock around the start and
// the join of all threads; it encloses fopen and the freads of the pieces, which are in the page cache after the first repeat.
#include "../../tools_src/defuse_host.hpp"

using namespace defuse;

struct Out { long long records = 0; unsigned long long check = 0; };

static void parse_sam(const char* path, Out& out)
{
    std::unordered_map<std::string, int> names;
    for (int k = 1; k <= 24; ++k) {
        char buf[16];
        snprintf(buf, sizeof buf, "chr%02d", k);
        names[buf] = k - 1;
    }
    FILE* f = fopen(path, "rb");
    if (!f) return;
    LineReader lr(f);
    const char* l;
    size_t n;
    int readEnd = -1;
    SamFields a;
    std::string reference;
    while (lr.next(l, n)) {
        const int kind = ParseSamLine(l, n, a, readEnd);
        if (kind == 1) continue;
        if (kind) break;
        int frag = -1;
        if (!field_int(a.fragment, a.fragment_len, frag)) frag = -1;
        reference.assign(a.reference, a.reference_len);
        const auto it = names.find(reference);
        ++out.records;
        out.check += (unsigned)(it == names.end() ? -1 : it->second) + (unsigned)a.region.start + (unsigned)a.region.end + (unsigned)frag + (unsigned)a.strand +
                     (unsigned)readEnd;
    }
    fclose(f);
}

static void parse_fastq(const char* path, Out& out)
{
    FastqReader in;
    std::ostringstream err;
    if (!in.open(path, err)) return;
    ReadStore store;
    FastqRecord r;
    while (in.next(r, err)) {
        int frag = 0;
        if (!field_int(r.fragment.data(), r.fragment.size(), frag)) break;
        store.put(frag, r.end, r.sequence.data(), r.sequence.size());
        ++out.records;
        out.check += (unsigned)frag + (unsigned)r.end + r.sequence.size();
    }
}

int main(int argc, char** argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: text_host sam|fastq <repeats> <piece> ...\n");
        return 2;
    }
    const std::string mode = argv[1];
    const int repeats = atoi(argv[2]);
    const int n = argc - 3;
    for (int rep = 0; rep < repeats; ++rep) {
        std::vector<Out> outs((size_t)n);
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int k = 0; k < n; ++k)
            th.emplace_back([&, k] { mode == "sam" ? parse_sam(argv[3 + k], outs[(size_t)k]) : parse_fastq(argv[3 + k], outs[(size_t)k]); });
        for (auto& t : th) t.join();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        Out all;
        for (const Out& o : outs) { all.records += o.records; all.check += o.check; }
        printf("%s threads %d ms %.3f records %lld check %llu\n", mode.c_str(), n, ms, all.records, all.check);
        fflush(stdout);
    }
    return 0;
}
