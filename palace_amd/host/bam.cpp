#include "bam.hpp"
#include "../csrc/bam_record.hpp"
#include "mapped_file.hpp"
#include "trace.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <chrono>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <thread>

namespace palace_host {

namespace {

uint32_t le32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

template <class F>
void parallel_for(size_t n, int threads, F f)
{
    threads = std::max(1, std::min<int>(threads, static_cast<int>(n ? n : 1)));
    if (threads == 1) { f(0, n, 0); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) {
        size_t a = n * t / threads, b = n * (t + 1) / threads;
        pool.emplace_back([=] { f(a, b, t); });
    }
    for (auto &th : pool) th.join();
}

}  // namespace

uint64_t name_key(const char *s, size_t n, uint64_t seed)
{
    return palace::name_key(reinterpret_cast<const uint8_t *>(s), 0, static_cast<int64_t>(n), seed);
}

void RawBuf::release()
{
    if (p) ::munmap(p, mapped);
    p = nullptr; n = mapped = 0;
}
void RawBuf::alloc(size_t bytes)
{
    release();
    const size_t huge = size_t{2} << 20;
    mapped = (bytes + huge) / huge * huge;
    void *m = ::mmap(nullptr, mapped, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) { mapped = 0; throw std::bad_alloc(); }
    p = static_cast<uint8_t *>(m);
    n = bytes;
    if (!std::getenv("PALACE_BAM_SMALL_PAGES")) ::madvise(p, mapped, MADV_HUGEPAGE);      // (a hint: refused or ignored, the stream is in 4 KiB pages as before)
}

void rekey(BamColumns &c, uint64_t seed)
{
    for (int64_t i = 0; i < c.n(); i++)
        c.qkey[i] = name_key(reinterpret_cast<const char *>(c.raw.data()) + c.qname_at[i], c.qname_len[i], seed);
}

// The loader as a pipeline (the reference streams the file through htslib, generate_graph.cpp:644):
//   inflate workers   take the BGZF members one by one off the front, so the inflated stream grows from the front; helpers
//                     (a device) take batches off the back;
//   the walker        one thread, started by load_bam_begin the moment the header's end is known: the record boundaries behind the
//                     inflate front (serial: a record's size is its first word), published in steps of 4 096 records (round 6 also had
//                     the inflate workers walk the stream ahead of it in 1 MiB segments: measured without gain, removed);
//   the decode        the inflate workers, as they run out of members, take chunks of 32 768 walked records and write their
//                     columns (sized for the most records the stream can hold; pages behind the real ones are never touched);
//   load_bam_begin    returns as soon as the members that hold the header are there and the header is parsed -- the caller
//                     can start what depends on the target names only (name ranks, FASTG keys) beside the rest;
//   load_bam_finish   waits for the walker, helps with the chunks that are left, cuts the columns to the records found and
//                     puts the chunks' SA items and match segments behind one another.
struct BamLoad : BackMembers {
    std::unique_ptr<MappedFile> file;
    std::vector<BgzfMember> bgzf;        // the file's members
    std::mutex claim_mu;                 // members [next_front, next_back) are nobody's yet
    size_t next_front = 0, next_back = 0;
    std::atomic<size_t> by_helpers{0};
    std::unique_ptr<std::atomic<uint8_t>[]> done;
    std::vector<std::thread> workers;
    std::atomic<bool> bad{false};
    BamColumns *c = nullptr;
    int threads = 1;
    size_t first_record = 0;             // offset of the first alignment record in the inflated stream
    int32_t n_ref = 0;

    // bytes of the inflated stream that are final: everything in front of the first member still missing.  Blocks
    // until at least `need` bytes are there (or everything that will ever come is).
    size_t wait_for(size_t need, size_t &ready_blocks)         // ready_blocks: the caller's own cursor (members [0, ready_blocks) seen inflated)
    {
        for (;;) {
            while (ready_blocks < bgzf.size() && done[ready_blocks].load(std::memory_order_acquire)) ready_blocks++;
            const size_t have = ready_blocks < bgzf.size() ? bgzf[ready_blocks].out_off : c->raw.size();
            if (have >= need || ready_blocks == bgzf.size()) return have;
            if (bad) throw std::runtime_error("BGZF inflate failed");
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    // the record walk (serial: a record's size is its first word; one step of it is walk_step of bam_record.hpp), on a thread of its own
    // from the moment the header's end is known
    std::thread walker;
    std::string walk_error;
    void walk();
    // the decode of the records into columns, pipelined behind the record walk (load_bam_finish): the walker publishes how many record
    // starts it has found, the loader's threads -- done with the inflate -- take chunks of records as they become known
    static constexpr size_t kChunk = 32768;
    std::vector<uint64_t> rec_at;        // reserved to the most records the stream can hold: never reallocated while it is read
    std::atomic<size_t> n_walked{0};
    std::atomic<bool> walk_done{false};
    std::atomic<int> decode_go{0};       // the name index is filled (SA items can be resolved): the decode may start
    std::atomic<size_t> next_chunk{0};
    uint64_t key_seed = 1;
    Column<int32_t> sa_cnt;
    std::vector<std::vector<palace_sa_item>> sa_part;      // per chunk, in record order
    std::vector<std::vector<int32_t>> ms_part;            // (tid, pos, len) triples per chunk
    void decode_range(size_t a, size_t b, size_t part);
    void decode_chunks();
    std::atomic<int> helpers_running{0};
    size_t hold_at = SIZE_MAX;           // tests (PALACE_BAM_HOST_SHARE=<per cent>): the threads stop there while a helper is at work
    bool claim_front(size_t *i)
    {
        for (;;) {
            {
                std::lock_guard<std::mutex> g(claim_mu);
                if (next_front >= next_back) return false;
                if (next_front < hold_at || helpers_running.load() == 0) { *i = next_front++; return true; }
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    // A helper's batch comes back after its transfer and decode latency (a device: ~20 ms for the slowest member of any batch, plus
    // the copies), in which the loader's threads get through some 1 500 members themselves: nothing of the last 1 500, and of what
    // is left two fifths per claim -- a device with two helper threads decodes ~3 x what sixteen host threads do, so it should end
    // up with about three quarters of what both start on (0.4 + 0.4 x 0.6 now, the same of what is left when a helper returns)
    bool claim(size_t max, size_t *first, size_t *n) override
    {
        std::lock_guard<std::mutex> g(claim_mu);
        const size_t left = next_back - next_front;
        if (bad || left < 1500) return false;
        *n = std::min(max, left * 2 / 5);
        next_back -= *n;
        *first = next_back;
        return true;
    }
    void finished(size_t i, bool decoded) override
    {
        if (!decoded && !inflate_member(file->bytes(), file->size, bgzf[i], c->raw.data() + bgzf[i].out_off)) bad = true;
        if (decoded) by_helpers.fetch_add(1, std::memory_order_relaxed);
        done[i].store(1, std::memory_order_release);
    }
    ~BamLoad() override
    {
        bad = true;                          // unwinding from a header / record error: the workers stop at their next member
        if (walker.joinable()) walker.join();
        for (auto &t : workers) if (t.joinable()) t.join();
    }
};

BamLoad *load_bam_begin(const std::string &path, int threads, BamColumns &c, const std::vector<MemberHelper> &helpers)
{
    Trace trh("bam/header");
    std::unique_ptr<BamLoad> L(new BamLoad());
    L->c = &c;
    L->threads = threads = std::max(1, threads);
    L->file.reset(new MappedFile(path, MapHint::sequential, "Failed to open BAM ", "Failed to read BAM "));
    size_t total = 0;
    L->bgzf = bgzf_members(L->file->bytes(), L->file->size, &total);
    c.raw.alloc(total);
    const size_t nb = L->bgzf.size();
    L->done.reset(new std::atomic<uint8_t>[nb ? nb : 1]);
    for (size_t i = 0; i < nb; i++) L->done[i].store(0, std::memory_order_relaxed);
    BamLoad *ld = L.get();
    L->next_back = nb;
    // (a helper costs a device context and its buffers: not for files the threads are done with before the HIP runtime is even up)
    if (!helpers.empty() && (nb >= 4096 || std::getenv("PALACE_BAM_HOST_SHARE"))) {
        L->members = L->bgzf.data();
        L->file_data = L->file->bytes();
        L->file_size = L->file->size;
        L->out = c.raw.data();
        if (const char *e = std::getenv("PALACE_BAM_HOST_SHARE")) L->hold_at = nb * static_cast<size_t>(std::max(0, std::min(100, std::atoi(e)))) / 100;
        L->helpers_running = static_cast<int>(helpers.size());
        for (const MemberHelper &h : helpers) L->workers.emplace_back([ld, h] { h(*ld); ld->helpers_running.fetch_sub(1); ld->decode_chunks(); });
    }
    for (int t = 0; t < threads; t++)
        L->workers.emplace_back([ld] {
            z_stream zs{};
            if (inflateInit2(&zs, -15) != Z_OK) { ld->bad = true; return; }
            uint8_t *out = ld->c->raw.data();
            const bool use_fast = std::getenv("PALACE_BAM_ZLIB") == nullptr;          // PALACE_BAM_ZLIB=1: zlib for every member (A/B, tests)
            for (size_t i = 0; !ld->bad && ld->claim_front(&i);) {
                const BgzfMember &m = ld->bgzf[i];
                if (!inflate_member(ld->file->bytes(), ld->file->size, m, out + m.out_off, &zs, use_fast)) { ld->bad = true; break; }
                ld->done[i].store(1, std::memory_order_release);
            }
            inflateEnd(&zs);
            ld->decode_chunks();
        });
    trh.lap("file mapped, members indexed, inflate threads started");
    // ---- header (BAM spec 4.2): magic, l_text, text, n_ref, then (l_name, name, l_ref) per reference ----
    const uint8_t *d = c.raw.data();
    size_t header_cursor = 0;
    auto need = [&](size_t upto) {
        if (L->wait_for(upto, header_cursor) < upto) throw std::runtime_error("Failed to read BAM header");
    };
    need(12);
    if (std::memcmp(d, "BAM\1", 4) != 0) throw std::runtime_error("Failed to read BAM header");
    size_t p = 8 + static_cast<size_t>(le32(d + 4));
    need(p + 4);
    const int32_t n_ref = static_cast<int32_t>(le32(d + p));
    p += 4;
    // (n_ref is bounded by what the stream can hold: >= 9 bytes per reference)
    const size_t cap = n_ref > 0 ? std::min<size_t>(static_cast<size_t>(n_ref), c.raw.size() / 9 + 1) : 0;
    std::vector<size_t> name_at;                                 // offset of every l_name word: a serial walk, each size is in the stream
    name_at.reserve(cap);
    for (int32_t i = 0; i < n_ref; i++) {
        need(p + 4);
        const size_t l = le32(d + p);
        need(p + 4 + l + 4);
        name_at.push_back(p);
        p += 8 + l;
    }
    trh.lap("name offsets walked (behind the inflate front)");
    // The end of the header is known: the record walk starts now, on a thread of its own, beside the rest of the header work (names,
    // hashes, the name index) -- the walk is the longest serial piece of the load (6.7 M dependent steps at 1M contigs).  The columns
    // are sized for the most records the stream can hold (36 bytes each at least; the pages behind the ones that do not exist are never
    // touched) so that the threads can decode chunks of records while the walk is still finding the later ones.
    L->first_record = p;
    L->n_ref = n_ref;
    {
        const size_t ub = (c.raw.size() > p ? (c.raw.size() - p) / 36 : 0) + 16;
        for (auto *v : {&c.tid, &c.pos, &c.mtid, &c.mpos, &c.nm, &c.ref_len, &c.read_len, &c.clip_s, &c.clip_e})
            v->resize(ub);
        c.flag.resize(ub); c.mapq.resize(ub); c.qkey.resize(ub);
        c.qname_at.resize(ub); c.qname_len.resize(ub);
        L->sa_cnt.resize(ub);
        const size_t max_chunks = ub / BamLoad::kChunk + 1;
        L->sa_part.resize(max_chunks);
        L->ms_part.resize(max_chunks);
        L->rec_at.reserve(ub);
        L->walker = std::thread([ld] { ld->walk(); });
    }
    // names, lengths and name hashes on the threads; the index itself is filled by this thread (hashes in hand)
    const size_t nr = name_at.size();
    c.target_name.resize(nr);
    c.target_len.resize(nr);
    std::vector<uint64_t> hash(nr);
    {
        const size_t parts = nr < 4096 ? 1 : static_cast<size_t>(std::min(threads, 8));
        std::vector<std::thread> pool;
        for (size_t t = 0; t < parts; t++)
            pool.emplace_back([&, t] {
                for (size_t i = nr * t / parts; i < nr * (t + 1) / parts; i++) {
                    const size_t at = name_at[i], l = le32(d + at);
                    const std::string_view nm(reinterpret_cast<const char *>(d + at + 4), l ? l - 1 : 0);
                    c.target_name[i].assign(nm);
                    c.target_len[i] = static_cast<int32_t>(le32(d + at + 4 + l));
                    hash[i] = hash_bytes(nm);
                }
            });
        for (auto &th : pool) th.join();
    }
    trh.lap("names, lengths, hashes (threads)");
    c.tid_names.reserve(nr + 16);
    c.tid_of_name.reserve(nr + 16);
    for (size_t i = 0; i < nr; i++) {
        if (i + 8 < nr) c.tid_names.prefetch(hash[i + 8]);
        const size_t at = name_at[i], l = le32(d + at);
        const int k = c.tid_names.intern_hashed(std::string_view(reinterpret_cast<const char *>(d + at + 4), l ? l - 1 : 0), hash[i]);
        if (static_cast<size_t>(k) >= c.tid_of_name.size()) c.tid_of_name.resize(static_cast<size_t>(k) + 1);
        c.tid_of_name[static_cast<size_t>(k)] = static_cast<int32_t>(i);
    }
    trh.lap("name index filled");
    L->decode_go.store(1, std::memory_order_release);            // the name index is there: SA items can be resolved
    return L.release();
}

size_t load_bam_size_hint(const BamLoad *load) { return load->c->raw.size(); }

void load_bam(const std::string &path, int threads, uint64_t key_seed, BamColumns &c)
{
    load_bam_finish(load_bam_begin(path, threads, c), key_seed);
}

void BamLoad::walk()
{
    const uint8_t *d = c->raw.data();
    const size_t total = c->raw.size();
    size_t cursor = 0;
    try {
        size_t p = first_record, have = wait_for(std::min(total, p + 4), cursor), ahead = p & ~size_t{63};
        for (;;) {
            int64_t next = 0;
            int st = palace::walk_step(d, static_cast<int64_t>(p), static_cast<int64_t>(have), static_cast<int64_t>(total), &next);
            if (st < 0) {                                             // behind the inflate front: wait for the bytes the step needs
                have = wait_for(std::min(total, p + 4), cursor);
                if (p + 4 <= have) have = wait_for(std::min(total, p + 4 + static_cast<size_t>(le32(d + p))), cursor);
                st = palace::walk_step(d, static_cast<int64_t>(p), static_cast<int64_t>(have), static_cast<int64_t>(total), &next);
                if (st < 0) break;                                    // (everything that will ever come is there, and it is not enough)
            }
            if (st == 0) break;
            rec_at.push_back(p + 4);
            if ((rec_at.size() & 4095) == 0) n_walked.store(rec_at.size(), std::memory_order_release);
            p = static_cast<size_t>(next);
            // the next few record heads lie in the kilobyte behind this one, not at a fixed stride (the hardware does not see a
            // stream): every line of that kilobyte is asked for as the walk exposes it
            for (const size_t upto = std::min(have, p + 1024); ahead + 64 <= upto; ahead += 64) __builtin_prefetch(d + ahead);
            if (ahead < p) ahead = p & ~size_t{63};
        }
    } catch (const std::exception &e) { walk_error = e.what(); }
    n_walked.store(rec_at.size(), std::memory_order_release);
    walk_done.store(true, std::memory_order_release);
}

// records [a, b) of the walk into the columns (every element written exactly once, by the thread that has the chunk): one pass per
// record, every rule a call into bam_record.hpp -- the text the kernels of csrc/bam.hip are compiled from
void BamLoad::decode_range(size_t a, size_t b, size_t part)
{
    using namespace palace;
    BamColumns &c = *this->c;
    const uint8_t *d = c.raw.data();
    const int32_t n_ref = this->n_ref;
    const uint64_t key_seed = this->key_seed;
    std::vector<int32_t> &ms = ms_part[part];
    std::vector<palace_sa_item> &sa = sa_part[part];
    auto view = [](const uint8_t *p, int64_t n) { return std::string_view(reinterpret_cast<const char *>(p), static_cast<size_t>(n)); };
    for (size_t i = a; i < b; i++) {
        const int64_t s = static_cast<int64_t>(rec_at[i]), end = s + static_cast<int64_t>(ld32(d, s - 4));
        const int32_t tid = static_cast<int32_t>(ld32(d, s));
        c.tid[i] = tid;
        c.pos[i] = static_cast<int32_t>(ld32(d, s + 4));
        c.mapq[i] = d[s + 9];
        c.flag[i] = static_cast<uint16_t>(ld16(d, s + 14));
        c.mtid[i] = static_cast<int32_t>(ld32(d, s + 20));
        c.mpos[i] = static_cast<int32_t>(ld32(d, s + 24));
        const int64_t nlen = name_len(d, s);
        c.qname_at[i] = static_cast<uint64_t>(s + 32);
        c.qname_len[i] = static_cast<uint8_t>(nlen);
        c.qkey[i] = palace::name_key(d, s + 32, nlen, key_seed);
        const RecCigar cg = record_cigar(d, s, end);
        const RecOps r = record_ops(d, s, cg, c.want_match_segments && depth_counts(d, s, n_ref),
                                    [&](int32_t t, int32_t pos, int32_t len) { ms.push_back(t); ms.push_back(pos); ms.push_back(len); });
        c.ref_len[i] = static_cast<int32_t>(r.ref_len);
        c.read_len[i] = static_cast<int32_t>(r.read_len);
        c.clip_s[i] = cg.n_ops ? r.sc.clip_s() : -1;
        c.clip_e[i] = r.sc.clip_e();
        const RecAux x = record_aux(d, cg.aux, end);               // one scan: the first NM and the first SA:Z
        c.nm[i] = x.nm;
        int32_t n_sa = 0;
        if (x.sa >= 0 && tid >= 0 && tid < n_ref) {                // :687
            const std::string &own = c.target_name[static_cast<size_t>(tid)];
            sa_text_items(d, x.sa, x.sa + x.sa_len, [&](const SaFields &f) {
                sa.push_back(sa_item(d, f, [&](const uint8_t *p, int64_t n) { return view(p, n) == own; },
                                     [&](const uint8_t *p, int64_t n) { return c.tid_of(view(p, n)); }));
                n_sa++;
            });
        }
        sa_cnt[i] = n_sa;
    }
}

void BamLoad::decode_chunks()
{
    while (!decode_go.load(std::memory_order_acquire)) {          // (the header is being parsed, or the loader is being torn down)
        if (bad) return;
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    for (;;) {
        const size_t part = next_chunk.fetch_add(1), a = part * kChunk;
        size_t have;
        for (;;) {
            const bool done = walk_done.load(std::memory_order_acquire);
            have = n_walked.load(std::memory_order_acquire);
            if (have >= a + kChunk || done) break;
            if (bad) return;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        if (a >= have || part >= sa_part.size()) return;
        decode_range(a, std::min(a + kChunk, have), part);
    }
}

void load_bam_finish(BamLoad *load, uint64_t key_seed)
{
    std::unique_ptr<BamLoad> L(load);
    BamColumns &c = *L->c;
    Trace tr("bam");
    L->walker.join();                                             // the record walk (started by load_bam_begin), behind the inflate front
    if (!L->walk_error.empty()) throw std::runtime_error(L->walk_error);
    std::vector<uint64_t> &rec_at = L->rec_at;
    tr.lap("record boundaries (behind the inflate front)");
    L->decode_chunks();                                           // this thread helps with what is left
    for (auto &t : L->workers) t.join();                          // (members behind a malformed record are still inflated)
    tr.lap("inflate threads joined, columns decoded");
    if (tr.on && L->members)                                      // (helpers were started)
        std::fprintf(stderr, "[bam] %zu of %zu members were inflated by helpers (device)\n", L->by_helpers.load(), L->bgzf.size());
    if (L->bad) throw std::runtime_error("BGZF inflate failed");
    L->file.reset();
    const size_t n = rec_at.size();
    for (auto *v : {&c.tid, &c.pos, &c.mtid, &c.mpos, &c.nm, &c.ref_len, &c.read_len, &c.clip_s, &c.clip_e})
        v->resize(n);
    c.flag.resize(n); c.mapq.resize(n); c.qkey.resize(n);
    c.qname_at.resize(n); c.qname_len.resize(n);
    c.sa_off.resize(n + 1);
    c.sa_off[0] = 0;
    const Column<int32_t> &sa_cnt = L->sa_cnt;
    for (size_t i = 0; i < n; i++) c.sa_off[i + 1] = c.sa_off[i] + sa_cnt[i];
    c.sa.clear();
    c.sa.reserve(static_cast<size_t>(c.sa_off[n]) + 1);
    for (auto &part : L->sa_part) c.sa.insert(c.sa.end(), part.begin(), part.end());   // chunks are in record order
    size_t n_ms = 0;
    for (auto &part : L->ms_part) n_ms += part.size() / 3;
    c.mseg_tid.reserve(n_ms); c.mseg_pos.reserve(n_ms); c.mseg_len.reserve(n_ms);
    for (auto &part : L->ms_part)
        for (size_t k = 0; k + 2 < part.size(); k += 3) { c.mseg_tid.push_back(part[k]); c.mseg_pos.push_back(part[k + 1]); c.mseg_len.push_back(part[k + 2]); }
    if (key_seed != L->key_seed) rekey(c, key_seed);             // (the decode keyed the read names with the default seed)
    tr.lap("SA items + match segments joined");
}

}  // namespace palace_host
