// task_cache.hpp — the split-read task set kept in a file next to the regions file (DEFUSE_DSA_TASK_CACHE=1).
//
// Every dosplitalign process of a run (one per read chunk) and the evalsplitalign after them build the same tasks from the
// same regions, FASTA, exon table and parameters (CreateTasks, defuse_host.hpp).  With the variable set, the first process
// whose set-up finished without a word writes what it built to "<regions>.dsatasks"; the others load that file instead.  A
// file is only used when the key it carries equals the key of the current inputs, its sizes hold together and its checksums
// match; anything else (no file, a damaged file, a directory in its place, a file that cannot be written) is a miss, and the
// cold path runs exactly as without the variable.  Nothing here prints unless DEFUSE_TIMING is set.  DESIGN.md, "Task cache".
//
// File: Header, then the payload —
//   int32 fusion id [n_tasks]                      (ascending), zero-padded to 8 bytes
//   uint64 record offset [n_tasks + 1]             (into the records; offset[0] = 0, offset[n_tasks] = records_bytes)
//   records [records_bytes]                        one per task, see put_task; zero-padded to 8 bytes
//   binned table [binned_bytes]                    BinnedLocations::Save of dosplitalign's mate-region bins, or nothing
// All integers in the machine's byte order (the header's tag says which, and the sizes of the types).
#pragma once
#include "defuse_host.hpp"

#include <sys/types.h>

namespace defuse {
namespace task_cache {

inline bool enabled()
{
    const char* e = std::getenv("DEFUSE_DSA_TASK_CACHE");
    return e && std::atoi(e) != 0;
}

inline std::string path_for(const std::string& regions) { return regions + ".dsatasks"; }

// ---- hashing: 64-bit, four lanes of multiply-rotate, blocks hashed side by side and the block hashes hashed again ---------
inline uint64_t mix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t hash_bytes(const void* data, size_t n, uint64_t seed)
{
    const unsigned char* p = (const unsigned char*)data;
    const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL;
    uint64_t h[4] = {seed + P1, seed ^ P2, seed - P1, ~seed};
    size_t i = 0;
    for (; i + 32 <= n; i += 32)
        for (int k = 0; k < 4; ++k) {
            uint64_t v;
            std::memcpy(&v, p + i + 8 * k, 8);
            h[k] = rotl64(h[k] ^ (v * P2), 31) * P1;
        }
    uint64_t t = (uint64_t)n * P1 + seed;
    for (; i < n; ++i) t = (t ^ p[i]) * P2;
    return mix64(h[0]) ^ rotl64(mix64(h[1]), 17) ^ rotl64(mix64(h[2]), 29) ^ rotl64(mix64(h[3]), 43) ^ mix64(t);
}
inline uint64_t hash_parallel(const char* p, size_t n, unsigned threads)
{
    const size_t B = (size_t)4 << 20;
    const size_t nb = (n + B - 1) / B;
    std::vector<uint64_t> hb(nb);
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, nb));
    run_threads(nt, [&](unsigned t) {
        for (size_t b = t; b < nb; b += nt) hb[b] = hash_bytes(p + b * B, std::min(B, n - b * B), b);
    });
    return hash_bytes(hb.data(), hb.size() * 8, (uint64_t)n);
}

// ---- the key --------------------------------------------------------------------------------------------------------------
struct FileStamp { uint64_t dev = 0, ino = 0, size = 0, mtime_ns = 0; };
struct Key {
    uint64_t regions_size = 0, regions_hash = 0;
    FileStamp fasta, fai, exons;
    uint64_t ufrag_bits = 0, sfrag_bits = 0;
    int64_t minread = 0, maxread = 0;
};
static_assert(sizeof(Key) == 2 * 8 + 3 * 32 + 4 * 8, "Key has no padding");

inline bool stamp(const std::string& path, FileStamp& s)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return false;
    s.dev = (uint64_t)st.st_dev;
    s.ino = (uint64_t)st.st_ino;
    s.size = (uint64_t)st.st_size;
    s.mtime_ns = (uint64_t)st.st_mtim.tv_sec * 1000000000ULL + (uint64_t)st.st_mtim.tv_nsec;
    return true;
}

// Everything of the key but the regions' content (set by the caller from the bytes it parses).  false: a stat failed —
// a miss, and the cold path says what the reference says about the missing file.
inline bool stamp_inputs(Key& k, const std::string& fasta, const std::string& exons, double ufrag, double sfrag, int minread,
                         int maxread, std::string& why)
{
    if (fasta.size() > 3 && fasta.compare(fasta.size() - 3, 3, ".rz") == 0) { why = "compressed FASTA"; return false; }
    if (!stamp(fasta, k.fasta)) { why = "cannot stat " + fasta; return false; }
    if (!stamp(fasta + ".fai", k.fai)) { why = "cannot stat " + fasta + ".fai"; return false; }
    if (!stamp(exons, k.exons)) { why = "cannot stat " + exons; return false; }
    std::memcpy(&k.ufrag_bits, &ufrag, 8);
    std::memcpy(&k.sfrag_bits, &sfrag, 8);
    k.minread = minread;
    k.maxread = maxread;
    return true;
}

// ---- the header -----------------------------------------------------------------------------------------------------------
constexpr char kMagic[8] = {'D', 'F', 'D', 'S', 'A', 'T', 'K', '\n'};
constexpr uint32_t kVersion = 1;
constexpr uint64_t kByteOrder = 0x0102030405060708ULL;
constexpr uint32_t kTypes = (uint32_t)(sizeof(int) | sizeof(long) << 4 | sizeof(size_t) << 8 | sizeof(double) << 12 | sizeof(Key) << 16);

struct Header {
    char magic[8];
    uint32_t version, types;
    uint64_t byte_order;
    Key key;
    uint64_t n_tasks, records_bytes, binned_bytes, payload_bytes;
    uint64_t payload_hash;
    uint64_t header_hash;                  // of every byte above
};
static_assert(sizeof(Header) == 8 + 8 + 8 + sizeof(Key) + 6 * 8, "Header has no padding");

inline uint64_t header_hash(const Header& h) { return hash_bytes(&h, offsetof(Header, header_hash), kVersion); }
inline size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

// ---- one task's record ------------------------------------------------------------------------------------------------------
// int32 align strand, window start, window length, split-sequence strand (per end), then per end: name, window sequence,
// remainder sequence (each uint32 length + bytes), uint32 number of mate regions, each: name, int32 strand, start, end.
inline size_t task_bytes(const SplitAlignmentTask& t)
{
    size_t n = 4 * 2 * 4;
    for (int ce = 0; ce < 2; ++ce) {
        n += 4 + t.mAlignRefName[ce].size() + 4 + t.mSplitAlignSeq[ce].size() + 4 + t.mSplitRemainderSeq[ce].size() + 4;
        for (const Location& l : t.mMateRegions[ce]) n += 4 + l.refName.size() + 3 * 4;
    }
    return n;
}
inline char* put_task(char* p, const SplitAlignmentTask& t)
{
    auto i32 = [&](int32_t v) { std::memcpy(p, &v, 4); p += 4; };
    auto str = [&](const auto& s) { i32((int32_t)s.size()); std::memcpy(p, s.data(), s.size()); p += s.size(); };
    for (int ce = 0; ce < 2; ++ce) { i32(t.mAlignStrand[ce]); i32(t.mSplitAlignSeqStart[ce]); i32(t.mSplitAlignSeqLength[ce]); i32(t.mSplitSeqStrand[ce]); }
    for (int ce = 0; ce < 2; ++ce) {
        str(t.mAlignRefName[ce]);
        str(t.mSplitAlignSeq[ce]);
        str(t.mSplitRemainderSeq[ce]);
        i32((int32_t)t.mMateRegions[ce].size());
        for (const Location& l : t.mMateRegions[ce]) { str(l.refName); i32(l.strand); i32(l.start); i32(l.end); }
    }
    return p;
}
inline bool get_task(const char* p, const char* end, SplitAlignmentTask& t)
{
    bool ok = true;
    auto i32 = [&]() { int32_t v = 0; if (end - p < 4) { ok = false; return v; } std::memcpy(&v, p, 4); p += 4; return v; };
    auto str = [&](std::string& s) {
        const uint32_t n = (uint32_t)i32();
        if (!ok || (size_t)(end - p) < n) { ok = false; return; }
        s.assign(p, n);
        p += n;
    };
    auto seq = [&](SeqText& s) {                        // a view into the mapping, not a copy
        const uint32_t n = (uint32_t)i32();
        if (!ok || (size_t)(end - p) < n) { ok = false; return; }
        s.view(p, n);
        p += n;
    };
    for (int ce = 0; ce < 2; ++ce) { t.mAlignStrand[ce] = i32(); t.mSplitAlignSeqStart[ce] = i32(); t.mSplitAlignSeqLength[ce] = i32(); t.mSplitSeqStrand[ce] = i32(); }
    for (int ce = 0; ce < 2 && ok; ++ce) {
        str(t.mAlignRefName[ce]);
        seq(t.mSplitAlignSeq[ce]);
        seq(t.mSplitRemainderSeq[ce]);
        const uint32_t n = (uint32_t)i32();
        if (!ok || n > (size_t)(end - p) / 16) return false;
        t.mMateRegions[ce].resize(n);
        for (Location& l : t.mMateRegions[ce]) {
            str(l.refName);
            l.strand = i32(); l.start = i32(); l.end = i32();
            if (l.strand != PlusStrand && l.strand != MinusStrand) ok = false;       // (an index of the bins' tables)
        }
    }
    return ok && p == end;
}

// ---- load -------------------------------------------------------------------------------------------------------------------
// true: `tasks` holds the cached set (and *binned the cached bins when the file has them and binned is given: *have_binned).
// false: a miss, `why` says why, `tasks` is empty.
inline bool load(const std::string& path, const Key& key, unsigned threads, std::map<int, SplitAlignmentTask>& tasks,
                 BinnedLocations* binned, bool* have_binned, size_t& file_bytes, std::string& why)
{
    tasks.clear();
    if (have_binned) *have_binned = false;
    const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) { why = errno == ENOENT ? "no cache file" : std::string("cannot open: ") + std::strerror(errno); return false; }
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); why = "not a regular file"; return false; }
    file_bytes = (size_t)st.st_size;
    if (file_bytes < sizeof(Header)) { close(fd); why = "truncated header"; return false; }
    void* m = mmap(nullptr, file_bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) { why = "cannot map"; return false; }
    // on a hit the mapping stays for the rest of the process: the tasks' sequences are views into it.  (Writers only ever
    // rename a finished file into place, so the file under a mapping is never cut short.)
    struct Unmap { void* m; size_t n; bool keep = false; ~Unmap() { if (!keep) munmap(m, n); } } unmap{m, file_bytes};
    const char* base = (const char*)m;
    Header h;
    std::memcpy(&h, base, sizeof h);
    if (std::memcmp(h.magic, kMagic, 8) != 0) { why = "bad magic"; return false; }
    if (h.version != kVersion || h.types != kTypes || h.byte_order != kByteOrder) { why = "other version or machine"; return false; }
    if (h.header_hash != header_hash(h)) { why = "header checksum"; return false; }
    if (std::memcmp(&h.key, &key, sizeof key) != 0) { why = "key differs (inputs changed)"; return false; }
    const uint64_t n = h.n_tasks;
    const size_t avail = file_bytes - sizeof(Header);
    if (h.payload_bytes != avail || n > avail / 12 || h.records_bytes > avail || h.binned_bytes > avail) { why = "truncated or sizes differ"; return false; }
    const size_t ids_at = 0, offs_at = pad8((size_t)n * 4), recs_at = offs_at + ((size_t)n + 1) * 8;
    const size_t bins_at = recs_at + pad8((size_t)h.records_bytes);
    if (bins_at + h.binned_bytes != avail) { why = "truncated or sizes differ"; return false; }
    const char* pay = base + sizeof(Header);
    if (hash_parallel(pay, avail, threads) != h.payload_hash) { why = "payload checksum"; return false; }

    std::vector<int32_t> ids((size_t)n);
    std::vector<uint64_t> off((size_t)n + 1);
    if (n > 0) std::memcpy(ids.data(), pay + ids_at, (size_t)n * 4);
    std::memcpy(off.data(), pay + offs_at, ((size_t)n + 1) * 8);
    if (off[0] != 0 || off[(size_t)n] != h.records_bytes) { why = "bad record table"; return false; }
    std::vector<SplitAlignmentTask*> slot((size_t)n);
    for (size_t k = 0; k < n; ++k) {
        if ((k > 0 && ids[k] <= ids[k - 1]) || off[k + 1] < off[k]) { tasks.clear(); why = "bad record table"; return false; }
        slot[k] = &tasks.emplace_hint(tasks.end(), ids[k], SplitAlignmentTask())->second;
        slot[k]->mFusionID = ids[k];
    }
    const char* recs = pay + recs_at;
    const unsigned nt = n < 64 ? 1u : std::max(1u, threads);
    std::atomic<bool> bad{false};
    run_threads(nt, [&](unsigned t) {
        for (size_t k = n * t / nt; k < n * (t + 1) / nt && !bad.load(std::memory_order_relaxed); ++k)
            if (!get_task(recs + off[k], recs + off[k + 1], *slot[k])) bad.store(true);
    });
    if (bad.load()) { tasks.clear(); why = "bad record"; return false; }
    if (binned && h.binned_bytes) {
        if (!binned->Load(pay + bins_at, (size_t)h.binned_bytes)) { tasks.clear(); why = "bad bin table"; return false; }
        if (have_binned) *have_binned = true;
    }
    unmap.keep = true;
    return true;
}

// ---- store ------------------------------------------------------------------------------------------------------------------
// Writes the set to a file of its own in the cache's directory and renames it into place (the last of several writers wins;
// they all write the same bytes).  false (why): nothing is left behind, the old cache file, if any, is untouched.
inline bool store(const std::string& path, const Key& key, unsigned threads, const std::map<int, SplitAlignmentTask>& tasks,
                  const BinnedLocations* binned, size_t& file_bytes, std::string& why)
{
    const size_t n = tasks.size();
    std::vector<const SplitAlignmentTask*> task(n);
    std::vector<uint64_t> off(n + 1, 0);
    {
        size_t k = 0;
        for (const auto& kv : tasks) task[k++] = &kv.second;
    }
    const unsigned nt = n < 64 ? 1u : std::max(1u, threads);
    run_threads(nt, [&](unsigned t) {
        for (size_t k = n * t / nt; k < n * (t + 1) / nt; ++k) off[k + 1] = task_bytes(*task[k]);
    });
    for (size_t k = 0; k < n; ++k) off[k + 1] += off[k];
    std::string bins;
    if (binned) binned->Save(bins);
    const size_t offs_at = pad8(n * 4), recs_at = offs_at + (n + 1) * 8, bins_at = recs_at + pad8((size_t)off[n]);
    const size_t payload = bins_at + bins.size();
    file_bytes = sizeof(Header) + payload;
    std::unique_ptr<char[]> buf(new (std::nothrow) char[file_bytes]);
    if (!buf) { why = "out of memory"; return false; }
    char* pay = buf.get() + sizeof(Header);
    std::memset(pay, 0, recs_at);
    std::memset(pay + bins_at - 8, 0, 8);                  // (the records' padding)
    {
        size_t k = 0;
        for (const auto& kv : tasks) { const int32_t id = kv.first; std::memcpy(pay + 4 * k++, &id, 4); }
    }
    std::memcpy(pay + offs_at, off.data(), (n + 1) * 8);
    run_threads(nt, [&](unsigned t) {
        for (size_t k = n * t / nt; k < n * (t + 1) / nt; ++k) put_task(pay + recs_at + off[k], *task[k]);
    });
    std::memcpy(pay + bins_at, bins.data(), bins.size());
    Header h{};                                           // (no padding: every byte is set)
    std::memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.types = kTypes;
    h.byte_order = kByteOrder;
    h.key = key;
    h.n_tasks = n;
    h.records_bytes = off[n];
    h.binned_bytes = bins.size();
    h.payload_bytes = payload;
    h.payload_hash = hash_parallel(pay, payload, threads);
    h.header_hash = header_hash(h);
    std::memcpy(buf.get(), &h, sizeof h);

    // "<cache>.<pid>.<clock>.part": unique per writer, never "*.tmp" (cmdrunner's own suffix for the files it renames)
    const std::string tmp = path + "." + std::to_string((long long)getpid()) + "." +
                            std::to_string((unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count()) + ".part";
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
    if (fd < 0) { why = std::string("cannot create a file beside it: ") + std::strerror(errno); return false; }
    size_t done = 0;
    while (done < file_bytes) {
        const ssize_t w = write(fd, buf.get() + done, file_bytes - done);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) { why = std::string("write: ") + (w < 0 ? std::strerror(errno) : "no progress"); break; }
        done += (size_t)w;
    }
    if (close(fd) != 0 && done == file_bytes) { why = std::string("close: ") + std::strerror(errno); done = 0; }
    if (done != file_bytes) { unlink(tmp.c_str()); return false; }
    if (rename(tmp.c_str(), path.c_str()) != 0) {
        why = std::string("rename: ") + std::strerror(errno);
        unlink(tmp.c_str());
        return false;
    }
    return true;
}

// ---- the set-up of the two tools ----------------------------------------------------------------------------------------------
// What both tools do around CreateTasks: read the regions file (its bytes are hashed for the key, then parsed — the same
// bytes), look the key up, else set up cold.  Without the variable, ReadAlignRegionPairs and CreateTasks run as they always
// did.  `tag` starts the DEFUSE_TIMING lines ("[dosplitalign]").
struct SetUp {
    bool on = false;                  // the variable is set (and the caller allows it)
    bool key_ok = false;              // every stat succeeded and the regions file was read
    bool hit = false;
    bool clean = false;               // cold: the set-up printed nothing
    bool have_binned = false;         // hit: the bins came from the file too
    Key key;
    std::string path, tag;
    bool timing = false;

    void line(const std::string& what) const
    {
        if (timing) std::cerr << tag << " task cache " << what << std::endl;
    }

    std::map<int, std::vector<Location>> read_regions(const std::string& regions_file, unsigned threads)
    {
        if (on) {
            MappedText text;
            struct stat st;
            // (a regular file only: "-" and pipes take the reference's path; the text is read once, hashed and parsed)
            if (stat(regions_file.c_str(), &st) == 0 && S_ISREG(st.st_mode) && text.try_load(regions_file, false)) {
                key.regions_size = text.size();
                key.regions_hash = hash_parallel(text.data(), text.size(), threads);
                key_ok = true;
                struct Buf : std::streambuf {
                    Buf(const char* b, size_t n) { char* p = const_cast<char*>(b); setg(p, p, p + n); }
                } sb(text.data() ? text.data() : "", text.size());
                std::istream in(&sb);
                return ReadAlignRegionPairs(in);
            }
        }
        return ReadAlignRegionPairs(regions_file);
    }

    std::map<int, SplitAlignmentTask> tasks(const std::string& fasta, const std::string& exons, double ufrag, double sfrag, int minread,
                                            int maxread, const std::map<int, std::vector<Location>>& regions, unsigned threads,
                                            BinnedLocations* binned)
    {
        std::map<int, SplitAlignmentTask> out;
        if (on) {
            const double t0 = now_s();
            std::string why = "regions file not readable as a file";
            size_t bytes = 0;
            if (key_ok) key_ok = stamp_inputs(key, fasta, exons, ufrag, sfrag, minread, maxread, why);
            if (key_ok && load(path, key, threads, out, binned, &have_binned, bytes, why)) {
                hit = true;
                line("hit: " + std::to_string(out.size()) + " tasks, " + std::to_string(bytes) + " bytes" + (have_binned ? " with bins" : "") +
                     ", " + secs(now_s() - t0));
                return out;
            }
            line("miss (" + why + ")");
        }
        return CreateTasks(fasta, exons, ufrag, sfrag, minread, maxread, regions, threads, &clean);
    }

    // after a cold set-up that printed nothing and ended in nothing: keep it (binned: the finished bins, or null)
    void keep(const std::map<int, SplitAlignmentTask>& tasks, const BinnedLocations* binned, unsigned threads) const
    {
        if (!on || hit) return;
        if (!key_ok || !clean) { line(std::string("not written (") + (key_ok ? "the set-up printed a message" : "no key") + ")"); return; }
        const double t0 = now_s();
        size_t bytes = 0;
        std::string why;
        if (store(path, key, threads, tasks, binned, bytes, why))
            line("written: " + std::to_string(bytes) + " bytes, " + secs(now_s() - t0));
        else
            line("not written (" + why + ")");
    }

    static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    static std::string secs(double s)
    {
        std::ostringstream o;
        o << s << " s";
        return o.str();
    }
};

}  // namespace task_cache
}  // namespace defuse
