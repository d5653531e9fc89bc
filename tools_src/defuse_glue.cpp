// defuse_glue — the text glue between the path's tools, one binary, one subcommand per
// reference script, same arguments, same input and output formats:
//
//   defuse_glue merge_clusters f1 f2 ...            scripts/merge_clusters.pl:9-33        (stdout)
//   defuse_glue get_align_regions                   scripts/get_align_regions.pl:14-53    (stdin -> stdout)
//   defuse_glue remove_duplicates <min_size>        scripts/remove_duplicates.pl:11-104   (stdin -> stdout)
//   defuse_glue filter_unmatched                    scripts/filter_unmatched.pl:16-50     (stdin -> stdout)
//   defuse_glue divide_sam_chr_pairs -t <trans> -p <prefix>   scripts/divide_sam_chr_pairs.pl:9-177 (stdin -> files + list on stdout)
//   defuse_glue sort_alignments [-o out] f1 f2 ...  the `sort -n -k 1` / `sort -m -n -k 1` of scripts/defuse_run.pl:528,533
//   defuse_glue cluster_regions <min_size> -c clusters_out -r regions_out [clusters]   remove_duplicates, then get_align_regions
//   defuse_glue calc_span_stats -c clusters -b breaks -s seqs   scripts/calc_span_stats.pl:37-126   (stdout)
//   defuse_glue span_stats -c clusters -b breaks -s seqs [-o out]   calc_span_stats on the GPU
//
// A symlink named after a script (merge_clusters.pl -> defuse_glue) selects the subcommand by its own name, so the
// pipeline's `$scripts_directory/<script>.pl` can point at it unchanged.  The script steps are host text work (the files are a
// few hundred MB and every step is one pass), they are here because these steps sit between clustermatepairs, setcover and
// dosplitalign and were the slowest links once those ran on the GPU.  Three steps have a device part: sort_alignments, the sort
// between dosplitalign and evalsplitalign on the record store of include/defuse_rec.h, cluster_regions, which does
// remove_duplicates and get_align_regions in one process on the cluster text section of include/defuse_task.h, and span_stats,
// which is calc_span_stats on that section and the span statistics section of include/defuse_ptext.h.
// Where a script's output order follows Perl's hash order (randomised per process), the canonical order of
// SURVEY 8(c) is used: ascending numeric ids, chromosome names in string order.
#include <chrono>

#include "../include/defuse_dsa.h"
#include "../include/defuse_ptext.h"
#include "../include/defuse_rec.h"
#include "../include/defuse_task.h"
#include "defuse_host.hpp"

using namespace defuse;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

class Out {
public:
    explicit Out(FILE* f) : f_(f) { buf_.reserve((1u << 22) + 4096); }
    ~Out() { flush(); }
    std::string& buf() { return buf_; }
    void maybe_flush() { if (buf_.size() > (1u << 22)) flush(); }
    void flush() { if (!buf_.empty()) { fwrite(buf_.data(), 1, buf_.size(), f_); buf_.clear(); } }
private:
    FILE* f_;
    std::string buf_;
};

// scripts/merge_clusters.pl: cluster ids renumbered consecutively over all files, a new id at every change of the
// first column and at every file boundary; the rest of each line is copied
int merge_clusters(int argc, char** argv)
{
    if (argc == 0) { std::cerr << "Usage merge_clusters clusters1 clusters2 ...\n"; return 1; }
    Out out(stdout);
    long long cluster_id = 0;
    for (int a = 0; a < argc; ++a) {
        FILE* in = fopen(argv[a], "rb");
        if (!in) die(std::string("Error: Unable to open ") + argv[a]);
        LineReader reader(in);
        const char* line;
        size_t len;
        bool have = false;
        long long prev = 0;
        Fields f;
        while (reader.next(line, len)) {
            split_fields(line, len, 2, f);
            const long long id = num(f, 0, "cluster id");
            if (have && prev != id) ++cluster_id;
            prev = id;
            have = true;
            append_int(out.buf(), cluster_id);
            out.buf().append(line + f.len(0), len - f.len(0));
            out.buf() += '\n';
            out.maybe_flush();
        }
        fclose(in);
        if (have) ++cluster_id;
    }
    return 0;
}

// scripts/get_align_regions.pl: per (cluster, end) the reference name and strand of its last line and the extent of all
// its alignments; clusters ascending, end 0 then 1; a cluster without exactly two ends is an error
int get_align_regions()
{
    ClusterPieces in;
    in.load("-");
    const std::string text = align_regions_text(in);
    if (!text.empty() && fwrite(text.data(), 1, text.size(), stdout) != text.size()) fail("Error: failed writing the regions");
    return 0;
}

// scripts/remove_duplicates.pl: inside a cluster, fragments whose pair of positions (start on '+', end on '-', one per
// cluster end) was seen already are dropped; a cluster is kept if at least min_cluster_size fragments remain.
// Fragments are visited in ascending order (the script: Perl hash order), so of a set of duplicates the smallest
// fragment index stays.
int remove_duplicates(int argc, char** argv)
{
    int min_size;
    if (argc < 1 || !field_int(argv[0], strlen(argv[0]), min_size)) { std::cerr << "Usage: remove_duplicates min_cluster_size < in_clusters > out_clusters\n"; return 1; }
    struct Line { long long frag; int ce; long long pos; const char* text; size_t len; };
    struct Frag { long long frag, pos[2]; const char* text[2]; size_t len[2]; };
    struct Piece {
        std::vector<Line> lines;                 // of the current cluster, in file order
        std::vector<Frag> frags;
        std::vector<size_t> by_pos;
        std::vector<char> keep;
        std::string out;
        bool have = false;
        long long current = 0;
    };
    const double t_start = now();
    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    ClusterPieces in;
    in.load("-");
    std::vector<Piece> part(in.pieces);
    // a cluster's fragments ascending (the script: Perl hash order), of a fragment's lines per end the last one; of the fragments
    // with one pair of positions the smallest stays
    auto emit = [&](Piece& pc) {
        std::stable_sort(pc.lines.begin(), pc.lines.end(), [](const Line& a, const Line& b) { return a.frag < b.frag; });
        pc.frags.clear();
        for (size_t i = 0; i < pc.lines.size();) {
            Frag fr{pc.lines[i].frag, {0, 0}, {nullptr, nullptr}, {0, 0}};
            size_t j = i;
            for (; j < pc.lines.size() && pc.lines[j].frag == fr.frag; ++j) {
                const Line& l = pc.lines[j];
                fr.pos[l.ce] = l.pos; fr.text[l.ce] = l.text; fr.len[l.ce] = l.len;
            }
            if (!fr.text[0] || !fr.text[1]) fail("Error: fragment " + std::to_string(fr.frag) + " lacks a cluster end");   // the script dies on the undefined value
            pc.frags.push_back(fr);
            i = j;
        }
        pc.by_pos.resize(pc.frags.size());
        for (size_t k = 0; k < pc.by_pos.size(); ++k) pc.by_pos[k] = k;
        std::sort(pc.by_pos.begin(), pc.by_pos.end(), [&](size_t a, size_t b) {
            const Frag &x = pc.frags[a], &y = pc.frags[b];
            if (x.pos[0] != y.pos[0]) return x.pos[0] < y.pos[0];
            if (x.pos[1] != y.pos[1]) return x.pos[1] < y.pos[1];
            return a < b;                                    // ascending fragment id
        });
        pc.keep.assign(pc.frags.size(), 0);
        size_t kept = 0;
        for (size_t k = 0; k < pc.by_pos.size(); ++k) {
            const Frag& x = pc.frags[pc.by_pos[k]];
            if (k == 0 || x.pos[0] != pc.frags[pc.by_pos[k - 1]].pos[0] || x.pos[1] != pc.frags[pc.by_pos[k - 1]].pos[1]) { pc.keep[pc.by_pos[k]] = 1; ++kept; }
        }
        if ((long long)kept * 2 >= 2LL * min_size)
            for (size_t k = 0; k < pc.frags.size(); ++k)
                if (pc.keep[k])
                    for (int e = 0; e < 2; ++e) { pc.out.append(pc.frags[k].text[e], pc.frags[k].len[e]); pc.out += '\n'; }
        pc.lines.clear();
    };
    for (unsigned t = 0; t < in.pieces; ++t) part[t].out.reserve(in.cut[t + 1] - in.cut[t] + 1);      // never more than came in
    in.run([&](unsigned t, const char* line, size_t len) {
        Piece& pc = part[t];
        Fields f;
        split_fields(line, len, 9, f);
        if (f.n < 8) fail("Error: cluster line with fewer than 8 fields");
        const long long id = num(f, 0, "cluster id"), ce = num(f, 1, "cluster end"), frag = num(f, 2, "fragment id");
        if (pc.have && pc.current != id) emit(pc);
        pc.current = id;
        pc.have = true;
        if (ce != 0 && ce != 1) return;                         // the script stores it and never looks at it again
        const long long pos = (f.len(5) == 1 && f.p[5][0] == '+') ? num(f, 6, "start") : num(f, 7, "end");
        pc.lines.push_back(Line{frag, (int)ce, pos, line, len});    // the text stays mapped
    }, [&](unsigned t) { if (part[t].have) emit(part[t]); });
    if (timing) std::cerr << "[remove_duplicates] " << in.pieces << " piece(s) done " << now() - t_start << " s" << std::endl;
    // a file behind stdout: every thread copies its piece's output to its place; anything else: one after the other
    struct stat st;
    const off_t base = lseek(STDOUT_FILENO, 0, SEEK_CUR);
    if (in.pieces > 1 && fstat(STDOUT_FILENO, &st) == 0 && S_ISREG(st.st_mode) && base >= 0 && !(fcntl(STDOUT_FILENO, F_GETFL) & O_APPEND)) {
        std::vector<off_t> at(in.pieces + 1, base);
        for (unsigned t = 0; t < in.pieces; ++t) at[t + 1] = at[t] + (off_t)part[t].out.size();
        std::vector<char> bad(in.pieces, 0);
        run_threads(in.pieces, [&](unsigned t) {
            const std::string& o = part[t].out;
            for (size_t done = 0; done < o.size();) {
                const ssize_t w = pwrite(STDOUT_FILENO, o.data() + done, o.size() - done, at[t] + (off_t)done);
                if (w <= 0) { bad[t] = 1; return; }
                done += (size_t)w;
            }
        });
        for (char b : bad)
            if (b) fail("Error: failed writing the clusters");
        (void)lseek(STDOUT_FILENO, at[in.pieces], SEEK_SET);
    } else {
        for (const Piece& pc : part)
            if (!pc.out.empty() && fwrite(pc.out.data(), 1, pc.out.size(), stdout) != pc.out.size()) fail("Error: failed writing the clusters");
    }
    if (timing) std::cerr << "[remove_duplicates] written " << now() - t_start << " s" << std::endl;
    return 0;
}

// qname =~ /(.*)\/([12])/ : the last "/1" or "/2" of the name
bool split_qname(const char* q, size_t n, size_t& frag_len, int& read_end)
{
    for (size_t k = n; k-- > 1;)
        if ((q[k] == '1' || q[k] == '2') && q[k - 1] == '/') { frag_len = k - 1; read_end = q[k] - '0'; return true; }
    return false;
}

// scripts/filter_unmatched.pl: the lines of a fragment (a run of equal numeric fragment ids) are kept if both read ends occur
int filter_unmatched()
{
    LineReader reader(stdin);
    Out out(stdout);
    const char* line;
    size_t len;
    Fields f;
    bool have = false, ends[3] = {false, false, false};
    long long current = 0;
    std::string held;
    auto emit = [&]() {
        if (ends[1] && ends[2]) { out.buf() += held; out.maybe_flush(); }
        held.clear();
        ends[1] = ends[2] = false;
    };
    while (reader.next(line, len)) {
        split_fields(line, len, 2, f);
        size_t fl;
        int re;
        if (!split_qname(f.p[0], f.len(0), fl, re)) die("Error: read name without /1 or /2: " + f.str(0));
        int frag;
        if (!field_int(f.p[0], fl, frag)) die("Error: fragment id is not a number: " + f.str(0));
        if (have && frag != current) emit();
        current = frag;
        have = true;
        ends[re] = true;
        held.append(line, len);
        held += '\n';
    }
    if (have) emit();
    return 0;
}

// scripts/divide_sam_chr_pairs.pl: compact spanning alignments (fragment, read end - 1, rname, strand, pos, pos + len(SEQ) - 1)
// of every fragment with both ends aligned, written to one file per sorted chromosome pair <prefix><chr1>-<chr2>; the list of
// files goes to stdout.  A transcript's chromosome comes from the -t table (gene, transcript, chromosome).
int divide_sam_chr_pairs(int argc, char** argv)
{
    std::string trans, prefix;
    for (int a = 0; a < argc; ++a) {
        const std::string t = argv[a];
        if ((t == "-t" || t == "--trans") && a + 1 < argc) trans = argv[++a];
        else if ((t == "-p" || t == "--prefix") && a + 1 < argc) prefix = argv[++a];
        else { std::cerr << "Usage: divide_sam_chr_pairs -t trans_chr_map -p prefix < sam\n"; return 1; }
    }
    if (trans.empty() || prefix.empty()) { std::cerr << "Usage: divide_sam_chr_pairs -t trans_chr_map -p prefix < sam\n"; return 1; }
    std::unordered_map<std::string, std::string> trans_chr;
    {
        FILE* in = fopen(trans.c_str(), "rb");
        if (!in) die("Error: Unable to open " + trans);
        LineReader reader(in);
        const char* line;
        size_t len;
        Fields f;
        while (reader.next(line, len)) {
            split_fields(line, len, 4, f);
            if (f.n < 3) continue;
            trans_chr[f.str(0) + "|" + f.str(1)] = f.str(2);
        }
        fclose(in);
    }
    // per output file: buffered text, appended to the file when it grows (the script: every 10000 alignments)
    struct Sink { std::string name, buf; bool created = false; };
    std::map<std::pair<std::string, std::string>, Sink> sinks;
    auto flush = [&](Sink& s) {
        FILE* o = fopen(s.name.c_str(), s.created ? "ab" : "wb");      // the first write replaces an old file (unlink in the script)
        if (!o) die("Error: Unable to write to " + s.name);
        fwrite(s.buf.data(), 1, s.buf.size(), o);
        fclose(o);
        s.created = true;
        s.buf.clear();
    };
    // the current fragment: per read end (1, 2) and chromosome the compact lines
    std::map<std::string, std::string> cur[3];
    auto process = [&]() {
        if (!cur[1].empty() && !cur[2].empty())
            for (const auto& c1 : cur[1])
                for (const auto& c2 : cur[2]) {
                    const bool fwd = c1.first <= c2.first;
                    Sink& s = sinks[fwd ? std::make_pair(c1.first, c2.first) : std::make_pair(c2.first, c1.first)];
                    if (s.name.empty()) s.name = prefix + (fwd ? c1.first : c2.first) + "-" + (fwd ? c2.first : c1.first);
                    s.buf += c1.second;
                    s.buf += c2.second;
                    if (s.buf.size() > (1u << 20)) flush(s);
                }
        cur[1].clear();
        cur[2].clear();
    };
    LineReader reader(stdin);
    const char* line;
    size_t len;
    Fields f;
    std::string current, key, rec;
    bool have = false;
    while (reader.next(line, len)) {
        if (len > 0 && line[0] == '@') continue;
        split_fields(line, len, 11, f);
        if (f.n < 10) die("Error: sam line with fewer than 10 fields");
        size_t fl;
        int re;
        if (!split_qname(f.p[0], f.len(0), fl, re)) die("Error: read name without /1 or /2: " + f.str(0));
        const long long flag = num(f, 1, "flag"), pos = num(f, 3, "position");
        if (have && (fl != current.size() || memcmp(current.data(), f.p[0], fl) != 0)) process();
        current.assign(f.p[0], fl);
        have = true;
        key.assign(f.p[2], f.len(2));
        auto tc = trans_chr.find(key);
        const std::string& chr = tc == trans_chr.end() ? key : tc->second;
        rec.assign(f.p[0], fl); rec += '\t';
        append_int(rec, re - 1); rec += '\t';
        rec += key; rec += '\t';
        rec += (flag & 0x10) ? '-' : '+'; rec += '\t';
        append_int(rec, pos); rec += '\t';
        append_int(rec, pos + (long long)f.len(9) - 1); rec += '\n';
        cur[re][chr] += rec;
    }
    if (have) process();
    Out out(stdout);
    for (auto& kv : sinks) {
        flush(kv.second);
        out.buf() += kv.first.first; out.buf() += '\t'; out.buf() += kv.first.second; out.buf() += '\t'; out.buf() += kv.second.name; out.buf() += '\n';
    }
    return 0;
}

// `LC_ALL=C sort -n -k 1 FILE...` of alignment files (splitreads.alignments chunks; scripts/defuse_run.pl:528,533 sorts each
// chunk and merges them) on the GPU: the text goes up in pieces (include/defuse_rec.h, "alignment text"), the record store
// sorts and prints, the sorted text comes down.  Only files of plain lines are sorted, because only their records print as
// their bytes: anything else is declined with status 3 and nothing written, so that a caller falls back to GNU sort
// (`defuse_glue sort_alignments -o OUT FILES || LC_ALL=C sort ...`).  A library failure, no GPU included, is status 1.
int sort_alignments(int argc, char** argv)
{
    const char* usage = "Usage: sort_alignments [-o out] alignments1 [alignments2 ...]\n";
    std::string out_name;
    std::vector<std::string> names;
    for (int a = 0; a < argc; ++a) {
        const std::string t = argv[a];
        if (t == "-o" || t == "--output") {
            if (a + 1 >= argc) { std::cerr << usage; return 1; }
            out_name = argv[++a];
        } else names.push_back(t);
    }
    if (names.empty()) { std::cerr << usage; return 1; }
    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    int64_t piece_bytes = (int64_t)1 << 30;
    if (const char* pb = std::getenv("DEFUSE_SORT_PIECE_BYTES")) {
        char* end = nullptr;
        const long long v = strtoll(pb, &end, 10);
        if (end == pb || *end || v < 1) die(std::string("Error: DEFUSE_SORT_PIECE_BYTES is not a positive number: ") + pb);
        piece_bytes = std::min<long long>(v, INT32_MAX);
    }
    auto finish = [](int rc) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        if (std::getenv("DEFUSE_FULL_EXIT")) exit(rc);      // under a profiler that writes its files at exit
        _exit(rc);                                          // no teardown of a runtime whose work is done
    };
    // the output: opened only when there is something to write, so a declined or failed run leaves OUT as it was
    auto write_out = [&](const char* p, size_t n) {
        if (out_name.empty()) {
            if (n && fwrite(p, 1, n, stdout) != n) die("Error: failed writing the sorted alignments");
            return;
        }
        const int fd = open(out_name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) die("Error: unable to write to " + out_name);
        for (size_t done = 0; done < n;) {
            const ssize_t w = write(fd, p + done, n - done);
            if (w <= 0) die("Error: failed writing " + out_name);
            done += (size_t)w;
        }
        if (close(fd) != 0) die("Error: failed writing " + out_name);
    };
    const double t0 = now();
    std::vector<MappedText> files(names.size());
    size_t total = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        if (!files[k].try_load(names[k], false)) die("Error: Unable to open " + names[k]);
        total += files[k].size();
    }
    const double t_map = now();
    if (total == 0) {                                       // nothing to sort: no device is touched
        write_out(nullptr, 0);
        return 0;
    }
    auto lib_failed = [&](const char* what, const char* err) { std::cerr << "Error: sorting on the GPU failed: " << what << ": " << err << std::endl; finish(1); };
    rect_ctx* ctx = nullptr;
    rec_store* store = nullptr;
    const int device = dsa_pick_device();
    if (rect_create(device, &ctx) != 0) lib_failed("rect_create", rect_last_error());
    if (rec_create(device, &store) != 0) lib_failed("rec_create", rec_last_error());
    auto decline = [&](const std::string& name, int64_t line, const std::string& why) {
        std::cerr << "sort_alignments: " << name << " line " << line << ": " << why << "; not sorted here, use LC_ALL=C sort -n -k 1" << std::endl;
        finish(3);
    };
    double upload_ms = 0, device_ms = 0;
    int64_t n_pieces = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        const MappedText& text = files[k];
        int64_t lines_before = 0;
        for (size_t pos = 0; pos < text.size();) {
            size_t hi = std::min(text.size(), pos + (size_t)piece_bytes);
            rect_result res;
            for (;;) {
                if (rect_add(ctx, store, (const uint8_t*)text.data() + pos, (int64_t)(hi - pos), hi == text.size() ? 1 : 0, &res) != 0)
                    lib_failed("rect_add", rect_last_error());
                if (res.consumed > 0 || res.stop_line || hi == text.size()) break;
                hi = text.line_end(hi);                     // a line longer than a piece goes up whole
            }
            ++n_pieces;
            if (timing) {
                rect_timing t;
                if (rect_get_timing(ctx, &t) == 0) { upload_ms += t.upload_ms; device_ms += t.device_ms; }
            }
            if (res.n_other) decline(names[k], lines_before + res.first_other, "the line is not what its record prints as (nine \"%d\\t\")");
            if (res.stop_line) {
                const std::string field = std::to_string(res.stop_field + 1);
                decline(names[k], lines_before + res.stop_line,
                        res.stop_kind == RECT_FEW_FIELDS ? "fewer than nine fields"
                        : res.stop_kind == RECT_BAD_BOOL ? "field " + field + " is not 0 or 1" : "field " + field + " is not an integer");
            }
            lines_before += res.n_lines;
            pos += (size_t)res.consumed;
        }
    }
    const double t_parse = now();
    if (rec_sort(store) != 0) lib_failed("rec_sort", rec_last_error());
    const double t_sort = now();
    // plain lines print as their own bytes: the text is the input and one newline per file that lacks its last one
    const int64_t cap = (int64_t)(total + names.size());
    std::unique_ptr<char[]> sorted(new char[(size_t)cap]);
    int64_t bytes = 0;
    if (rec_text(store, nullptr, 0, sorted.get(), cap, &bytes) != 0) lib_failed("rec_text", rec_last_error());
    const double t_text = now();
    write_out(sorted.get(), (size_t)bytes);
    const double t_write = now();
    if (timing) {
        rec_timing t{};
        (void)rec_get_timing(store, &t);
        std::cerr << "[sort_alignments] " << names.size() << " file(s), " << total << " bytes, " << t.n_records << " records in " << n_pieces
                  << " piece(s): map " << t_map - t0 << " s, upload+parse " << t_parse - t_map << " s, sort " << t_sort - t_parse
                  << " s, print+download " << t_text - t_sort << " s, write " << t_write - t_text << " s\n"
                  << "[sort_alignments] device: upload " << upload_ms << " ms, tables+parse " << device_ms << " ms, keys " << t.keys_ms << " ms, sorts "
                  << t.sort_ms << " ms (" << t.n_sorts << "), permute " << t.gather_ms << " ms, format " << t.format_ms << " ms, download " << t.download_ms
                  << " ms" << std::endl;
    }
    finish(0);
    return 0;
}

// remove_duplicates and get_align_regions in one process on the GPU (include/defuse_task.h, "cluster text"): the cluster file
// goes up in pieces, CLUSTERS_OUT is what `remove_duplicates MIN` prints and REGIONS_OUT what `get_align_regions` prints of
// it.  Anything either host step would die of is declined with status 3 and neither file touched, so that a caller falls
// back (`defuse_glue cluster_regions MIN -c C -r R FILE || { the two host steps; }`) and gets the host's message.  A library
// failure, no GPU included, is status 1 with nothing written.
int cluster_regions(int argc, char** argv)
{
    const char* usage = "Usage: cluster_regions min_cluster_size -c clusters_out -r regions_out [clusters]\n";
    std::string clusters_out, regions_out, in_name = "-";
    std::vector<std::string> plain;
    for (int a = 0; a < argc; ++a) {
        const std::string t = argv[a];
        if ((t == "-c" || t == "-r") && a + 1 >= argc) { std::cerr << usage; return 1; }
        if (t == "-c") clusters_out = argv[++a];
        else if (t == "-r") regions_out = argv[++a];
        else plain.push_back(t);
    }
    int min_size = 0;
    if (plain.empty() || plain.size() > 2 || clusters_out.empty() || regions_out.empty() || !field_int(plain[0].data(), plain[0].size(), min_size)) {
        std::cerr << usage;
        return 1;
    }
    if (plain.size() == 2) in_name = plain[1];
    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    int64_t piece_bytes = (int64_t)1 << 30;
    if (const char* pb = std::getenv("DEFUSE_GLUE_PIECE_BYTES")) {
        char* end = nullptr;
        const long long v = strtoll(pb, &end, 10);
        if (end == pb || *end || v < 1) die(std::string("Error: DEFUSE_GLUE_PIECE_BYTES is not a positive number: ") + pb);
        piece_bytes = std::min<long long>(v, INT32_MAX);
    }
    auto finish = [](int rc) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        if (std::getenv("DEFUSE_FULL_EXIT")) exit(rc);      // under a profiler that writes its files at exit
        _exit(rc);                                          // no teardown of a runtime whose work is done
    };
    auto lib_failed = [&](const char* what, const char* err) { std::cerr << "Error: cluster_regions on the GPU failed: " << what << ": " << err << std::endl; finish(1); };
    const double t0 = now();
    MappedText text;
    if (!text.try_load(in_name, true, false)) die("Error: Unable to open clusters file " + in_name);
    const double t_map = now();
    taskc_ctx* ctx = nullptr;
    if (taskc_create(dsa_pick_device(), &ctx) != 0) lib_failed("taskc_create", taskc_last_error());
    if (taskc_begin(ctx) != 0) lib_failed("taskc_begin", taskc_last_error());
    for (size_t pos = 0; pos < text.size();) {
        size_t hi = std::min(text.size(), pos + (size_t)piece_bytes);
        int64_t consumed = 0;
        for (;;) {
            if (taskc_add(ctx, (const uint8_t*)text.data() + pos, (int64_t)(hi - pos), hi == text.size() ? 1 : 0, &consumed) != 0)
                lib_failed("taskc_add", taskc_last_error());
            if (consumed > 0 || hi == text.size()) break;
            hi = text.line_end(hi);                         // a line longer than a piece goes up whole
        }
        pos += (size_t)consumed;
    }
    const double t_up = now();
    auto decline = [&](const char* step, const taskc_result& r) {
        std::cerr << "cluster_regions: " << step;
        if (r.stop_line) std::cerr << " line " << r.stop_line;
        if (r.stop_kind == TASKC_FEW_FIELDS) std::cerr << ": fewer than eight fields";
        else if (r.stop_kind == TASKC_BAD_INTEGER) std::cerr << ": field " << r.stop_field + 1 << " is not an integer";
        else if (r.stop_kind == TASKC_MISSING_END) std::cerr << ": fragment " << r.stop_value << " of the cluster that ends here lacks a cluster end";
        else std::cerr << ": cluster " << r.stop_value << " does not have two ends";
        std::cerr << "; nothing written, use remove_duplicates and get_align_regions" << std::endl;
        finish(3);
    };
    taskc_result dres, rres;
    if (taskc_dedup(ctx, (int64_t)min_size, &dres) != 0) lib_failed("taskc_dedup", taskc_last_error());
    if (dres.stop_kind) decline("clusters", dres);
    if (taskc_regions(ctx, TASKC_DEDUP, &rres) != 0) lib_failed("taskc_regions", taskc_last_error());
    if (rres.stop_kind) decline("kept clusters", rres);
    const double t_dev = now();
    std::unique_ptr<uint8_t[]> clusters(new uint8_t[(size_t)dres.out_bytes + 1]), regions(new uint8_t[(size_t)rres.out_bytes + 1]);
    if (taskc_fetch(ctx, TASKC_DEDUP, 0, clusters.get(), dres.out_bytes) != 0) lib_failed("taskc_fetch", taskc_last_error());
    if (taskc_fetch(ctx, TASKC_REGIONS, 0, regions.get(), rres.out_bytes) != 0) lib_failed("taskc_fetch", taskc_last_error());
    const double t_down = now();
    auto write_file = [&](const std::string& name, const uint8_t* p, size_t n) {
        const int fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) die("Error: unable to write to " + name);
        for (size_t done = 0; done < n;) {
            const ssize_t w = write(fd, p + done, n - done);
            if (w <= 0) die("Error: failed writing " + name);
            done += (size_t)w;
        }
        if (close(fd) != 0) die("Error: failed writing " + name);
    };
    write_file(clusters_out, clusters.get(), (size_t)dres.out_bytes);
    write_file(regions_out, regions.get(), (size_t)rres.out_bytes);
    const double t_write = now();
    if (timing) {
        taskc_timing t{};
        (void)taskc_get_timing(ctx, &t);
        std::cerr << "[cluster_regions] " << text.size() << " bytes, " << dres.n_lines << " lines in " << t.n_pieces << " piece(s), " << dres.n_runs << " runs, "
                  << dres.n_fragments << " fragments (" << dres.n_kept_fragments << " kept), " << rres.n_clusters << " clusters: map " << t_map - t0
                  << " s, create+upload " << t_up - t_map << " s, dedup+regions " << t_dev - t_up << " s, download " << t_down - t_dev << " s, write "
                  << t_write - t_down << " s\n"
                  << "[cluster_regions] device: upload " << t.upload_ms << " ms, tables " << t.tables_ms << " ms, parse " << t.parse_ms << " ms, sorts " << t.sorts_ms
                  << " ms, select " << t.select_ms << " ms, gather " << t.gather_ms << " ms, regions " << t.regions_ms << " ms, print " << t.print_ms << " ms"
                  << std::endl;
    }
    finish(0);
    return 0;
}

// -c/--clusters, -b/--breaks, -s/--seqs (and -o/--output where `out` is given) of the two span statistics steps
bool span_arguments(int argc, char** argv, std::string& clusters, std::string& breaks, std::string& seqs, std::string* out)
{
    for (int a = 0; a < argc; ++a) {
        const std::string t = argv[a];
        std::string* into = (t == "-c" || t == "--clusters") ? &clusters : (t == "-b" || t == "--breaks") ? &breaks : (t == "-s" || t == "--seqs") ? &seqs
                            : (out && (t == "-o" || t == "--output")) ? out : nullptr;
        if (!into || a + 1 >= argc) return false;
        *into = argv[++a];
    }
    return !clusters.empty() && !breaks.empty() && !seqs.empty();
}

// scripts/calc_span_stats.pl by the rules of include/defuse_ptext.h, "span statistics": per cluster with a break entry the
// mean length of its spanning fragments up to the break and their number, "%d\t%.15g\t%lld\n", clusters ascending (the script:
// Perl hash order).  Of every (cluster, end) the strand of its last line, of every (cluster, fragment, end) the positions of its
// last line, of every key of the two small files its last line.  Anything that stops prints nothing and is status 1.
int calc_span_stats(int argc, char** argv)
{
    std::string clusters_name, breaks_name, seqs_name;
    if (!span_arguments(argc, argv, clusters_name, breaks_name, seqs_name, nullptr)) {
        std::cerr << "Usage: calc_span_stats -c clusters -b breaks -s seqs > span_stats\n";
        return 1;
    }
    const long long max_coord = TASK_MAX_COORD;
    auto each_line = [](const MappedText& text, const std::function<void(size_t, const char*, size_t)>& fn) {
        size_t n = 0;
        for (size_t pos = 0; pos < text.size(); ++n) {
            const char* nl = (const char*)memchr(text.data() + pos, '\n', text.size() - pos);
            const size_t end = nl ? (size_t)(nl - text.data()) : text.size();
            fn(n + 1, text.data() + pos, end - pos);
            pos = end + 1;
        }
    };
    auto line_stop = [](const std::string& name, size_t line, const std::string& why) { die("Error: " + name + " line " + std::to_string(line) + ": " + why); };
    auto integer = [&](const std::string& name, size_t line, const Fields& f, int k) {
        int v = 0;
        if (!field_int(f.p[k], f.len(k), v)) line_stop(name, line, "field " + std::to_string(k + 1) + " is not an integer");
        return v;
    };
    MappedText breaks, seqs, clusters;
    if (!breaks.try_load(breaks_name, false)) die("Error: Unable to find " + breaks_name);
    if (!seqs.try_load(seqs_name, false)) die("Error: Unable to find " + seqs_name);
    if (!clusters.try_load(clusters_name, false)) die("Error: Unable to find " + clusters_name);
    std::map<std::pair<int, int>, int> break_pos;
    std::unordered_map<int, int> inter;
    Fields f;
    each_line(breaks, [&](size_t n, const char* line, size_t len) {
        split_fields(line, len, 6, f);
        if (f.n < 5) line_stop(breaks_name, n, "fewer than five fields");
        const int id = integer(breaks_name, n, f, 0), end = integer(breaks_name, n, f, 1);
        break_pos[{id, end}] = integer(breaks_name, n, f, 4);
    });
    each_line(seqs, [&](size_t n, const char* line, size_t len) {
        split_fields(line, len, 4, f);
        if (f.n < 3) line_stop(seqs_name, n, "fewer than three fields");
        const int id = integer(seqs_name, n, f, 0);
        inter[id] = integer(seqs_name, n, f, 2);
    });
    struct Line { int id, frag, ce; const char* strand; const char* start; const char* end; uint32_t strand_len, start_len, end_len; };
    std::vector<Line> lines;
    std::unordered_map<uint64_t, uint32_t> end_last;        // (id, end) -> its last line
    each_line(clusters, [&](size_t n, const char* line, size_t len) {
        split_fields(line, len, 9, f);
        if (f.n < 8) line_stop(clusters_name, n, "fewer than eight fields");
        const int id = integer(clusters_name, n, f, 0), ce = integer(clusters_name, n, f, 1), frag = integer(clusters_name, n, f, 2);
        end_last[((uint64_t)(uint32_t)id << 32) | (uint32_t)ce] = (uint32_t)lines.size();
        lines.push_back(Line{id, frag, ce, f.p[5], f.p[6], f.p[7], (uint32_t)f.len(5), (uint32_t)f.len(6), (uint32_t)f.len(7)});
    });
    std::vector<uint32_t> order(lines.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (uint32_t)k;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const Line &x = lines[a], &y = lines[b];
        return x.id != y.id ? x.id < y.id : x.frag != y.frag ? x.frag < y.frag : x.ce < y.ce;
    });
    std::string out;
    char buf[96];
    for (size_t lo = 0; lo < order.size();) {
        const int id = lines[order[lo]].id;
        size_t hi = lo;
        while (hi < order.size() && lines[order[hi]].id == id) ++hi;
        const auto first = break_pos.lower_bound({id, INT_MIN});
        if (first == break_pos.end() || first->first.first != id) {            // the script: next if not defined
            lo = hi;
            continue;
        }
        // what stops the cluster, the first of the header's list
        int rank = 7, bad_field = 0;
        auto stop = [&](int r, int field = 0) { if (r < rank || (r == rank && field < bad_field)) { rank = r; bad_field = field; } };
        std::vector<int> ends;
        for (size_t k = lo; k < hi; ++k) ends.push_back(lines[order[k]].ce);
        std::sort(ends.begin(), ends.end());
        if (std::unique(ends.begin(), ends.end()) - ends.begin() != 2) stop(1);
        long long sum = 0, count = 0;
        for (size_t k = lo; k < hi; ++k) {
            const Line& l = lines[order[k]];
            if (k == lo || lines[order[k - 1]].frag != l.frag) ++count;
            if (k + 1 < hi && lines[order[k + 1]].frag == l.frag && lines[order[k + 1]].ce == l.ce) continue;      // not the last of its (fragment, end)
            const Line& s = lines[end_last[((uint64_t)(uint32_t)id << 32) | (uint32_t)l.ce]];
            const bool plus = s.strand_len == 1 && s.strand[0] == '+';
            const auto b = break_pos.find({id, l.ce});
            if (b == break_pos.end()) stop(2);
            else if (b->second > max_coord || b->second < -max_coord) stop(4);
            int pos = 0;
            if (!field_int(plus ? l.start : l.end, plus ? l.start_len : l.end_len, pos)) stop(3, plus ? 7 : 8);
            else if (pos > max_coord || pos < -max_coord) stop(4);
            if (rank == 7) sum += plus ? (long long)b->second - pos + 1 : (long long)pos - b->second + 1;
        }
        const auto in = inter.find(id);
        if (in == inter.end()) stop(5);
        else if (in->second > max_coord || in->second < -max_coord) stop(4);
        else sum += (long long)in->second * count;
        if (rank == 7 && (sum > (1ll << 53) || sum < -(1ll << 53))) stop(6);
        if (rank == 1) die("Error: Did not find 2 reference names for cluster " + std::to_string(id));
        if (rank < 7) {
            const std::string why = rank == 2   ? "a cluster end has no entry in " + breaks_name
                                    : rank == 3 ? "field " + std::to_string(bad_field) + " of a line whose position is used is not an integer"
                                    : rank == 4 ? "a break, a position or the inter length is beyond +-" + std::to_string(max_coord)
                                    : rank == 5 ? "the cluster has no entry in " + seqs_name
                                                : "the sum of the fragment lengths is beyond 2^53";
            die("Error: " + clusters_name + " cluster " + std::to_string(id) + ": " + why);
        }
        const int n = snprintf(buf, sizeof buf, "%d\t%.15g\t%lld\n", id, (double)sum / (double)count, count);
        out.append(buf, (size_t)n);
        lo = hi;
    }
    if (!out.empty() && fwrite(out.data(), 1, out.size(), stdout) != out.size()) die("Error: failed writing the span statistics");
    return 0;
}

// calc_span_stats on the GPU (include/defuse_ptext.h, "span statistics"): the cluster file goes up in pieces through the cluster
// text section, the two small files whole, OUT (or stdout) is what `calc_span_stats` prints.  Anything the host step would die of,
// and a text whose key fields are not all plain "%d" (Perl keys its hashes by their bytes), is declined with status 3 and OUT
// not touched, so that a caller falls back (`defuse_glue span_stats ... -o OUT || defuse_glue calc_span_stats ... > OUT`).  A
// library failure, no GPU included, is status 1 with nothing written.
int span_stats_tool(int argc, char** argv)
{
    std::string clusters_name, breaks_name, seqs_name, out_name;
    if (!span_arguments(argc, argv, clusters_name, breaks_name, seqs_name, &out_name)) {
        std::cerr << "Usage: span_stats -c clusters -b breaks -s seqs [-o out]\n";
        return 1;
    }
    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    int64_t piece_bytes = (int64_t)1 << 30;
    if (const char* pb = std::getenv("DEFUSE_GLUE_PIECE_BYTES")) {
        char* end = nullptr;
        const long long v = strtoll(pb, &end, 10);
        if (end == pb || *end || v < 1) die(std::string("Error: DEFUSE_GLUE_PIECE_BYTES is not a positive number: ") + pb);
        piece_bytes = std::min<long long>(v, INT32_MAX);
    }
    auto finish = [](int rc) {
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        if (std::getenv("DEFUSE_FULL_EXIT")) exit(rc);      // under a profiler that writes its files at exit
        _exit(rc);                                          // no teardown of a runtime whose work is done
    };
    auto lib_failed = [&](const char* what, const char* err) { std::cerr << "Error: span_stats on the GPU failed: " << what << ": " << err << std::endl; finish(1); };
    const double t0 = now();
    MappedText clusters, breaks, seqs;
    if (!breaks.try_load(breaks_name, false)) die("Error: Unable to find " + breaks_name);
    if (!seqs.try_load(seqs_name, false)) die("Error: Unable to find " + seqs_name);
    if (!clusters.try_load(clusters_name, false, false)) die("Error: Unable to find " + clusters_name);
    const double t_map = now();
    const int device = dsa_pick_device();
    taskc_ctx* text = nullptr;
    span_ctx* ctx = nullptr;
    if (taskc_create(device, &text) != 0) lib_failed("taskc_create", taskc_last_error());
    if (span_create(device, &ctx) != 0) lib_failed("span_create", span_last_error());
    if (taskc_begin(text) != 0) lib_failed("taskc_begin", taskc_last_error());
    for (size_t pos = 0; pos < clusters.size();) {
        size_t hi = std::min(clusters.size(), pos + (size_t)piece_bytes);
        int64_t consumed = 0;
        for (;;) {
            if (taskc_add(text, (const uint8_t*)clusters.data() + pos, (int64_t)(hi - pos), hi == clusters.size() ? 1 : 0, &consumed) != 0)
                lib_failed("taskc_add", taskc_last_error());
            if (consumed > 0 || hi == clusters.size()) break;
            hi = clusters.line_end(hi);                     // a line longer than a piece goes up whole
        }
        pos += (size_t)consumed;
    }
    const double t_up = now();
    auto decline = [&](const span_result& r) {
        std::cerr << "span_stats";
        if (r.stop_kind) std::cerr << ": " << (r.stop_file == SPAN_FILE_BREAKS ? breaks_name : r.stop_file == SPAN_FILE_SEQS ? seqs_name : clusters_name);
        if (r.stop_line) std::cerr << " line " << r.stop_line;
        else if (r.stop_kind) std::cerr << " cluster " << r.stop_value;
        if (r.stop_kind == SPAN_FEW_FIELDS) std::cerr << ": too few fields";
        else if (r.stop_kind == SPAN_BAD_INTEGER) std::cerr << ": field " << r.stop_field + 1 << " is not an integer";
        else if (r.stop_kind == SPAN_NOT_TWO_ENDS) std::cerr << ": not two cluster ends";
        else if (r.stop_kind == SPAN_NO_BREAK_END) std::cerr << ": a cluster end without a break";
        else if (r.stop_kind == SPAN_COORD_LIMIT) std::cerr << ": a coordinate beyond +-" << TASK_MAX_COORD;
        else if (r.stop_kind == SPAN_NO_INTER) std::cerr << ": no inter length";
        else if (r.stop_kind == SPAN_SUM_LIMIT) std::cerr << ": a sum beyond 2^53";
        else std::cerr << ": " << r.n_noncanonical << " key field(s) not in plain decimal";
        std::cerr << "; nothing written, use calc_span_stats" << std::endl;
        finish(3);
    };
    span_result bres, sres;
    if (span_breaks_text(ctx, (const uint8_t*)breaks.data(), (int64_t)breaks.size(), (const uint8_t*)seqs.data(), (int64_t)seqs.size(), &bres) != 0)
        lib_failed("span_breaks_text", span_last_error());
    if (bres.stop_kind) decline(bres);
    if (span_stats(ctx, text, TASKC_INPUT, &sres) != 0) lib_failed("span_stats", span_last_error());
    if (sres.stop_kind) decline(sres);
    sres.n_noncanonical += bres.n_noncanonical;
    if (sres.n_noncanonical) decline(sres);
    const double t_dev = now();
    std::unique_ptr<span_row[]> rows(new span_row[(size_t)sres.n_rows + 1]);
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[(size_t)sres.out_bytes + 1]);
    if (span_fetch(ctx, rows.get(), sres.n_rows, bytes.get(), sres.out_bytes) != 0) lib_failed("span_fetch", span_last_error());
    const double t_down = now();
    if (out_name.empty()) {
        if (sres.out_bytes && fwrite(bytes.get(), 1, (size_t)sres.out_bytes, stdout) != (size_t)sres.out_bytes) die("Error: failed writing the span statistics");
    } else {
        const int fd = open(out_name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (fd < 0) die("Error: unable to write to " + out_name);
        for (size_t done = 0; done < (size_t)sres.out_bytes;) {
            const ssize_t w = write(fd, bytes.get() + done, (size_t)sres.out_bytes - done);
            if (w <= 0) die("Error: failed writing " + out_name);
            done += (size_t)w;
        }
        if (close(fd) != 0) die("Error: failed writing " + out_name);
    }
    const double t_write = now();
    if (timing) {
        span_timing t{};
        taskc_timing tc{};
        (void)span_get_timing(ctx, &t);
        (void)taskc_get_timing(text, &tc);
        std::cerr << "[span_stats] " << clusters.size() << " bytes, " << sres.n_lines << " lines in " << tc.n_pieces << " piece(s), " << bres.n_breaks << " breaks, "
                  << sres.n_ids << " clusters, " << sres.n_rows << " rows: map " << t_map - t0 << " s, create+upload " << t_up - t_map << " s, tables+stats "
                  << t_dev - t_up << " s, download " << t_down - t_dev << " s, write " << t_write - t_down << " s\n"
                  << "[span_stats] device: upload " << tc.upload_ms << " ms, line tables " << tc.tables_ms << " ms, parse " << tc.parse_ms << " ms, breaks upload "
                  << t.upload_ms << " ms, lines " << t.lines_ms << " ms, tables " << t.tables_ms << " ms, sorts " << t.sorts_ms << " ms, terms " << t.terms_ms
                  << " ms, print " << t.print_ms << " ms, download " << t.download_ms << " ms" << std::endl;
    }
    finish(0);
    return 0;
}

}  // namespace

int main(int argc, char* argv[])
{
    std::string prog = argc > 0 ? argv[0] : "";
    const size_t slash = prog.find_last_of('/');
    if (slash != std::string::npos) prog = prog.substr(slash + 1);
    if (prog.size() > 3 && prog.compare(prog.size() - 3, 3, ".pl") == 0) prog.resize(prog.size() - 3);
    int first = 1;
    if (prog == "defuse_glue") {
        if (argc < 2) {
            std::cerr << "Usage: defuse_glue merge_clusters|get_align_regions|remove_duplicates|filter_unmatched|divide_sam_chr_pairs|calc_span_stats|sort_alignments|"
                         "cluster_regions|span_stats [args]\n";
            return 1;
        }
        prog = argv[1];
        first = 2;
    }
    try {
        if (prog == "merge_clusters") return merge_clusters(argc - first, argv + first);
        if (prog == "get_align_regions") return get_align_regions();
        if (prog == "remove_duplicates") return remove_duplicates(argc - first, argv + first);
        if (prog == "filter_unmatched") return filter_unmatched();
        if (prog == "divide_sam_chr_pairs") return divide_sam_chr_pairs(argc - first, argv + first);
        if (prog == "sort_alignments") return sort_alignments(argc - first, argv + first);
        if (prog == "cluster_regions") return cluster_regions(argc - first, argv + first);
        if (prog == "calc_span_stats") return calc_span_stats(argc - first, argv + first);
        if (prog == "span_stats") return span_stats_tool(argc - first, argv + first);
    } catch (const GlueError& g) {
        die(g.msg);
    }
    std::cerr << "defuse_glue: unknown subcommand " << prog << "\n";
    return 1;
}
