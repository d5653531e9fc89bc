// estislands — drop-in replacement of the reference's EST island filter (tools/estislands.cpp, tools/EstCatalog.cpp): same
// command line (-e EST alignments, -b breakpoint alignments, -o output), same messages and exit status, and the same output:
// every breakpoint alignment that lies inside an island of merged EST alignments padded by 300 bases, as read, in input order.
// The text is parsed on the host (the EST table in pieces on DEFUSE_THREADS threads); the islands are built and searched on
// the GPU (include/defuse_est.h).  There is no CPU fallback: without a HIP device a run that has something to look up exits 1.
//
// Two deviations: where the reference dies of an uncaught bad_lexical_cast this tool prints an `Error:`
// line and exits 1 — before the output file exists for the EST table, after the contained lines before the bad row for the
// breakpoint file — and segments are merged in the canonical order (chromosome, start, input order), which decides the
// islands where the reference's unstable std::sort would leave them to chance (rows with tEnd <= tStart only).
#include "../include/defuse_dsa.h"
#include "../include/defuse_est.h"
#include "defuse_host.hpp"

using namespace defuse;

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the columns of a used row: chromosome, tStart, tEnd
struct Layout { int chrom, start, end; };
constexpr Layout EST_FIELDS{14, 16, 17};       // tools/EstCatalog.cpp:46-58: UCSC intronEst with its leading bin column
constexpr Layout BREAK_FIELDS{13, 15, 16};     // :126-138: blat -noHead PSL

// the chromosome name as the reference keys it: a leading "chr" removed, then "M" -> "MT"
inline std::string_view chrom_key(std::string_view f)
{
    if (f.size() >= 3 && f.compare(0, 3, "chr") == 0) f.remove_prefix(3);
    if (f == "M") return "MT";
    return f;
}

// the used rows of one piece of a text: what the reference reads from its lines (tools/EstCatalog.cpp:24-58, 110-138)
struct Piece {
    std::vector<int32_t> chrom, start, end;
    std::vector<size_t> line_off, line_len;     // breakpoint rows only: the line as read
    std::vector<std::string> names;             // local chromosome ids -> names, in order of first use (EST rows)
    size_t lines = 0;                           // lines in the piece
    bool bad = false;                           // the first unparsable row of the piece ends it
    size_t bad_line = 0;                        // its line number within the piece (1-based)
    std::string bad_field;
};

// Parses the lines of text[lo, hi).  names_in == nullptr: chromosome names get local ids (EST table); else they are looked up
// and unknown ones get -1 (breakpoint file).
void parse_piece(const char* text, size_t lo, size_t hi, const Layout& L, const std::unordered_map<std::string, int>* names_in, Piece& out)
{
    std::unordered_map<std::string, int> local;
    std::string name;
    std::string_view last_name;
    int last_id = -2;
    Fields f, g;
    size_t pos = lo;
    while (pos < hi) {
        const char* line = text + pos;
        const char* nl = (const char*)memchr(line, '\n', hi - pos);
        const size_t len = nl ? (size_t)(nl - line) : hi - pos;
        pos += len + (nl ? 1 : 0);
        ++out.lines;
        if (len == 0 || line[0] < '0' || line[0] > '9') continue;          // empty lines, '#' and other headers
        // boost::split on every tab: at least 18 fields; the last one keeps a '\r' (fields L.chrom.. 18 are split off the tail,
        // so that field 17 ends at a tab if there is one)
        split_fields(line, len, L.chrom + 1, f);
        if (f.n < L.chrom + 1) continue;
        const char* tail = f.p[L.chrom];
        split_fields(tail, (size_t)(line + len - tail), 19 - L.chrom, g);
        if (g.n < 18 - L.chrom) continue;
        int s, e;
        const int ks = L.start - L.chrom, ke = L.end - L.chrom;
        if (!field_int(g.p[ks], g.len(ks), s)) { out.bad = true; out.bad_line = out.lines; out.bad_field = g.str(ks); return; }
        if (!field_int(g.p[ke], g.len(ke), e)) { out.bad = true; out.bad_line = out.lines; out.bad_field = g.str(ke); return; }
        const std::string_view key = chrom_key(std::string_view(g.p[0], g.len(0)));
        int id;
        if (last_id != -2 && key == last_name) {
            id = last_id;
        } else {
            name.assign(key.data(), key.size());
            if (names_in) {
                auto it = names_in->find(name);
                id = it == names_in->end() ? -1 : it->second;
            } else {
                auto it = local.find(name);
                if (it == local.end()) {
                    it = local.emplace(name, (int)out.names.size()).first;
                    out.names.push_back(name);
                }
                id = it->second;
            }
            last_name = key;              // (points into the text, which outlives the piece)
            last_id = id;
        }
        out.chrom.push_back(id);
        out.start.push_back((int32_t)((uint32_t)s + 1u));      // int(tStart) + 1, wrapping as the reference's int addition does
        out.end.push_back(e);
        if (names_in) {
            out.line_off.push_back((size_t)(line - text));
            out.line_len.push_back(len);
        }
    }
}

// A named input as ifstream opens it: "-" is a file of that name, a directory opens and reads as empty.  false: cannot open.
bool load_text(const std::string& name, MappedText& text)
{
    const int fd = open(name.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    const bool dir = fstat(fd, &st) == 0 && S_ISDIR(st.st_mode);
    close(fd);
    if (dir) return true;
    return text.try_load(name, false, false);
}

// the pieces of a whole text parsed on a team; the first bad row in file order and its 1-based line number
struct Parsed {
    std::vector<Piece> pieces;
    int bad_piece = -1;
    size_t bad_line = 0;
};

Parsed parse_text(Team& team, const MappedText& text, const Layout& L, const std::unordered_map<std::string, int>* names_in)
{
    Parsed r;
    const unsigned nt = text.size() < ((size_t)1 << 20) ? 1u : team.size();
    const std::vector<size_t> cut = text.cut_lines(0, text.size(), nt);
    r.pieces.resize(nt);
    team.run([&](unsigned t) {
        if (t < nt) parse_piece(text.data(), cut[t], cut[t + 1], L, names_in, r.pieces[t]);
    });
    size_t lines = 0;
    for (unsigned t = 0; t < nt; ++t) {
        if (r.pieces[t].bad) { r.bad_piece = (int)t; r.bad_line = lines + r.pieces[t].bad_line; break; }
        lines += r.pieces[t].lines;
    }
    return r;
}

std::string bad_integer(const Parsed& p, const char* what, const std::string& file)
{
    return "Error: bad integer '" + p.pieces[(size_t)p.bad_piece].bad_field + "' in " + what + " " + file + " line " + std::to_string(p.bad_line);
}

}  // namespace

int main(int argc, char* argv[])
{
    CmdLine cmd("Identify products of cotranscribed regions using est islands");
    cmd.add("e", "ests", "EST Alignments Filename", "string");
    cmd.add("b", "breaks", "Breakpoint Alignments Filename", "string");
    cmd.add("o", "output", "Output Filtered Alignments Filename", "string");
    cmd.parse(argc, argv);
    const std::string est_name = cmd.str("ests"), break_name = cmd.str("breaks"), out_name = cmd.str("output");

    const bool timing = std::getenv("DEFUSE_TIMING") != nullptr;
    double t_stage = now();
    auto stage = [&](const char* name) {
        const double t = now();
        if (timing) std::cerr << "[estislands] " << name << " " << (t - t_stage) << " s" << std::endl;
        t_stage = t;
    };
    Team team(host_threads());

    // ---- the EST table (tools/estislands.cpp:42-52): pieces with local chromosome ids, merged into dense global ids ----
    std::unordered_map<std::string, int> chrom_id;
    std::vector<int32_t> chrom, start, end;
    {
        MappedText text;
        if (!load_text(est_name, text)) die("Error: Unable to open est file " + est_name);
        Parsed p = parse_text(team, text, EST_FIELDS, nullptr);
        if (p.bad_piece >= 0) die(bad_integer(p, "est file", est_name));      // reference: uncaught bad_lexical_cast
        const size_t np = p.pieces.size();
        std::vector<std::vector<int32_t>> remap(np);
        std::vector<size_t> at(np + 1, 0);
        for (size_t t = 0; t < np; ++t) {
            for (const std::string& nm : p.pieces[t].names) {
                auto it = chrom_id.emplace(nm, (int)chrom_id.size()).first;
                remap[t].push_back(it->second);
            }
            at[t + 1] = at[t] + p.pieces[t].chrom.size();
        }
        chrom.resize(at[np]);
        start.resize(at[np]);
        end.resize(at[np]);
        team.run([&](unsigned t) {
            if (t >= np) return;
            const Piece& pc = p.pieces[t];
            for (size_t k = 0; k < pc.chrom.size(); ++k) chrom[at[t] + k] = remap[t][(size_t)pc.chrom[k]];
            std::copy(pc.start.begin(), pc.start.end(), start.begin() + (ptrdiff_t)at[t]);
            std::copy(pc.end.begin(), pc.end.end(), end.begin() + (ptrdiff_t)at[t]);
        });
    }

    // ---- the breakpoint alignments (:54-59), parsed whole before anything else can fail ----
    MappedText breaks;
    if (!load_text(break_name, breaks)) die("Error: Unable to open break alignments file " + break_name);
    {
        // the output is opened (truncated) after the breaks file: a breaks file that IS the output reads as empty
        struct stat sb, so;
        if (breaks.size() && stat(out_name.c_str(), &so) == 0 && stat(break_name.c_str(), &sb) == 0 && sb.st_dev == so.st_dev && sb.st_ino == so.st_ino)
            breaks.release();
    }
    Parsed q = parse_text(team, breaks, BREAK_FIELDS, &chrom_id);
    stage("read+parse");
    FILE* out = fopen(out_name.c_str(), "wb");                 // (:61-66)
    if (!out) die("Error: Unable to open output file " + out_name);

    // the rows before the first bad one are looked up (:103-173)
    const size_t np = q.bad_piece >= 0 ? (size_t)q.bad_piece + 1 : q.pieces.size();
    std::vector<size_t> at(np + 1, 0);
    for (size_t t = 0; t < np; ++t) at[t + 1] = at[t] + q.pieces[t].chrom.size();
    const size_t nq = at[np];
    std::vector<int32_t> qc(nq), qs(nq), qe(nq);
    for (size_t t = 0; t < np; ++t) {
        std::copy(q.pieces[t].chrom.begin(), q.pieces[t].chrom.end(), qc.begin() + (ptrdiff_t)at[t]);
        std::copy(q.pieces[t].start.begin(), q.pieces[t].start.end(), qs.begin() + (ptrdiff_t)at[t]);
        std::copy(q.pieces[t].end.begin(), q.pieces[t].end.end(), qe.begin() + (ptrdiff_t)at[t]);
    }
    std::vector<uint8_t> contained(nq, 0);
    est_timing et{};
    bool known = false;
    for (int32_t c : qc) known = known || c >= 0;
    if (known && !chrom.empty()) {                               // else nothing can be contained: no device is opened
        const int device = dsa_pick_device();                    // as the other tools: DEFUSE_GPU, else pid mod device count
        est_catalog* cat = nullptr;
        if (est_catalog_create(device, chrom.data(), start.data(), end.data(), (int64_t)chrom.size(), (int32_t)chrom_id.size(), &cat) != 0)
            die(std::string("Error: GPU EST catalogue failed: ") + est_last_error());
        stage("catalogue");
        if (est_catalog_contained(cat, qc.data(), qs.data(), qe.data(), (int64_t)nq, contained.data(), &et) != 0)
            die(std::string("Error: GPU EST island lookup failed: ") + est_last_error());
        est_catalog_destroy(cat);
        stage("lookup");
    } else {
        stage("catalogue");
        stage("lookup");
    }

    std::string buf;
    size_t k = 0;
    for (size_t t = 0; t < np; ++t) {
        const Piece& pc = q.pieces[t];
        for (size_t r = 0; r < pc.chrom.size(); ++r, ++k) {
            if (!contained[k]) continue;
            buf.append(breaks.data() + pc.line_off[r], pc.line_len[r]);
            buf.push_back('\n');
            if (buf.size() >= ((size_t)1 << 22)) { fwrite(buf.data(), 1, buf.size(), out); buf.clear(); }
        }
    }
    fwrite(buf.data(), 1, buf.size(), out);
    const bool write_ok = fflush(out) == 0 && !ferror(out);
    fclose(out);
    stage("write");
    if (timing)
        std::cerr << "[estislands] " << chrom.size() << " est rows (" << et.n_degenerate << " with end < start), " << et.n_islands << " islands, "
                  << nq << " break rows, " << et.n_contained << " contained; device build " << et.build_ms << " ms, lookup " << et.lookup_ms
                  << " ms" << std::endl;
    if (q.bad_piece >= 0) die(bad_integer(q, "break alignments file", break_name));     // reference: uncaught bad_lexical_cast
    if (!write_ok) die("Error: writing output file " + out_name + " failed");
    return 0;
}
