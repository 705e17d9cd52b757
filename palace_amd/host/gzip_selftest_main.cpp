// gzip_selftest: the device gzip inflater's host logic on a CPU, and a driver of palace_gzip_inflate that returns from main.
//   gzip_selftest blocks FILE                 the DEFLATE block starts of every member, found with zlib (Z_BLOCK): one line per block
//                                             "<bit of the file> <BTYPE> <BFINAL>", then "blocks N dynamic_nonfinal D"
//   gzip_selftest chain FILE STRIDE SPAN      gz_chain_walk (gzip_member.hpp) over spans of the file without a device: the candidates are
//                                             the true dynamic block starts a finder would report per stride (every fifth one moved a
//                                             few bits: a false hit), the size pass is zlib from a bit position; the chunks on the chain
//                                             must add up to zlib's text, member for member.  With a fifth argument `reach` the size
//                                             pass also reports how far a chunk reaches before its own start (the smallest preset
//                                             dictionary zlib decodes it with), and a file zlib refuses for a distance too far back
//                                             must be declined by the walk: "declined: 11"
//   gzip_selftest inflate FILE [STRIDE SPAN]  palace_gzip_inflate on the file, its text against zlib's (CRC-32 and length), the counters
//                                             and stage times; the driver for `rocprofv3 --kernel-trace --stats` (eref leaves through _exit)
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "gzip_member.hpp"

using namespace palace_host;

static std::vector<uint8_t> read_file(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// raw inflate from bit `bit` of file[0 .. limit) with Z_BLOCK: stops at the first block boundary at or after `stop` or behind a final
// block; the unknown window is `window` bytes of zeros (lengths and positions do not depend on it; a match that reaches further back
// than `window` is zlib's "invalid distance too far back")
static GzResult zlib_size(const uint8_t *file, int64_t limit, int64_t bit, int64_t stop, int window = 32768)
{
    GzResult r{0, bit, 0, kGzOk, 0};
    z_stream zs{};
    if (inflateInit2(&zs, -15) != Z_OK) { r.status = 2; return r; }
    static const std::vector<uint8_t> zeros(32768, 0);
    if (window > 0) inflateSetDictionary(&zs, zeros.data(), static_cast<uInt>(window));
    int64_t byte = bit >> 3;
    const int k = static_cast<int>(bit & 7);
    if (byte >= limit) { inflateEnd(&zs); r.status = kGzNeedsInput; return r; }
    if (k) { inflatePrime(&zs, 8 - k, file[byte] >> k); byte++; }
    zs.next_in = const_cast<Bytef *>(file + byte);
    zs.avail_in = static_cast<uInt>(limit - byte);
    std::vector<uint8_t> out(1 << 16);
    for (;;) {
        zs.next_out = out.data(); zs.avail_out = static_cast<uInt>(out.size());
        const int rc = inflate(&zs, Z_BLOCK);
        r.out_len += static_cast<int64_t>(out.size() - zs.avail_out);
        const int64_t pos = (static_cast<int64_t>(zs.next_in - file)) * 8 - (zs.data_type & 63);
        if (rc == Z_STREAM_END) { r.end_bit = pos; r.fin = 1; break; }
        if (rc == Z_BUF_ERROR || (rc == Z_OK && zs.avail_in == 0 && !(zs.data_type & 128))) {
            if (zs.avail_out == 0) continue;
            r.status = kGzNeedsInput; break;
        }
        if (rc != Z_OK) { r.status = 2; break; }
        if ((zs.data_type & 128) && (zs.data_type & 64) && pos > bit) { r.end_bit = pos; r.fin = 1; break; }   // the end of the last block
        if ((zs.data_type & 128) && pos > bit && pos >= stop) { r.end_bit = pos; break; }
    }
    inflateEnd(&zs);
    return r;
}

// ... and with the chunk's reach before its own start: the smallest window zlib decodes it with (by bisection)
static GzResult zlib_size_reach(const uint8_t *file, int64_t limit, int64_t bit, int64_t stop)
{
    GzResult r = zlib_size(file, limit, bit, stop);
    if (r.status != kGzOk) return r;
    int lo = 0, hi = 32768;                                                     // decodes with hi, not with any window below lo
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (zlib_size(file, limit, bit, stop, mid).status == kGzOk) hi = mid; else lo = mid + 1;
    }
    r.reach = lo;
    return r;
}

struct Block { int64_t bit; int btype, bfinal; };

static std::vector<Block> block_starts(const std::vector<uint8_t> &f)
{
    std::vector<Block> blocks;
    const int64_t size = static_cast<int64_t>(f.size());
    int64_t hdr = gzip_header_end(f.data(), f.size(), 0);
    while (hdr >= 0) {
        int64_t bit = hdr * 8;
        for (;;) {
            const uint32_t three = (f[bit >> 3] | (bit / 8 + 1 < size ? f[(bit >> 3) + 1] << 8 : 0)) >> (bit & 7);
            blocks.push_back(Block{bit, static_cast<int>((three >> 1) & 3), static_cast<int>(three & 1)});
            const GzResult r = zlib_size(f.data(), size, bit, bit + 1);
            if (r.status != kGzOk) { std::fprintf(stderr, "zlib refuses the block at bit %lld\n", static_cast<long long>(bit)); std::exit(1); }
            bit = r.end_bit;
            if (r.fin) break;
        }
        const int64_t next = ((bit + 7) >> 3) + 8;
        hdr = next < size ? gzip_header_end(f.data(), f.size(), static_cast<size_t>(next)) : -1;
    }
    return blocks;
}

static int run_chain(const std::vector<uint8_t> &f, int64_t stride, int64_t span, bool with_reach)
{
    const int64_t size = static_cast<int64_t>(f.size());
    const std::vector<Block> blocks = block_starts(f);
    // zlib's text length per member
    std::vector<uint64_t> want_len;
    bool too_far_back = false;
    for (size_t pos = 0; pos < f.size() && !too_far_back;) {
        z_stream zs{};
        inflateInit2(&zs, 31);
        zs.next_in = const_cast<Bytef *>(f.data() + pos); zs.avail_in = static_cast<uInt>(f.size() - pos);
        std::vector<uint8_t> out(1 << 16);
        int rc;
        uint64_t n = 0;
        do { zs.next_out = out.data(); zs.avail_out = static_cast<uInt>(out.size()); rc = inflate(&zs, Z_NO_FLUSH); n += out.size() - zs.avail_out; } while (rc == Z_OK);
        if (with_reach && rc == Z_DATA_ERROR && zs.msg && !std::strcmp(zs.msg, "invalid distance too far back")) { inflateEnd(&zs); too_far_back = true; break; }
        if (rc != Z_STREAM_END) { std::fprintf(stderr, "zlib refuses the file\n"); return 1; }
        pos = static_cast<size_t>(zs.next_in - f.data());
        inflateEnd(&zs);
        want_len.push_back(n);
    }
    int64_t cur_abs = gzip_header_end(f.data(), f.size(), 0) * 8;
    GzChainState cs{0, 1, false};
    std::vector<uint64_t> got_len;
    uint64_t member = 0;
    int64_t spans = 0, accepted = 0, found = 0, false_made = 0;
    while (!cs.file_done) {
        const int64_t a = (cur_abs >> 3) & ~int64_t{3}, b = std::min(size, a + span), end_bits = (b - a) * 8, rel = a * 8;
        spans++;
        std::vector<GzChunk> ch{GzChunk{cur_abs - rel, end_bits, 0, 0, 0, 0}};
        size_t bi = 0;
        for (int64_t c = 1; c * stride < b - a; c++) {                           // what the finder reports: the first start in every stride
            const int64_t lo = rel + c * stride * 8, hi = std::min(rel + (c + 1) * stride * 8, rel + end_bits);
            while (bi < blocks.size() && blocks[bi].bit < lo) bi++;
            size_t k = bi;
            while (k < blocks.size() && blocks[k].bit < hi && !(blocks[k].btype == 2 && !blocks[k].bfinal)) k++;
            if (k == blocks.size() || blocks[k].bit >= hi) continue;
            int64_t h = blocks[k].bit - rel;
            if (found % 5 == 4 && h - 3 >= lo - rel) { h -= 3; false_made++; }    // a false hit in front of the true start
            found++;
            if (h > ch.back().start) { ch.back().stop = h; ch.push_back(GzChunk{h, end_bits, 0, 0, 0, 0}); }
        }
        std::vector<GzResult> res;
        for (const GzChunk &c : ch) {
            GzResult r = with_reach ? zlib_size_reach(f.data() + a, b - a, c.start, c.stop) : zlib_size(f.data() + a, b - a, c.start, c.stop);
            res.push_back(r);
        }
        std::vector<GzAccepted> acc;
        const GzSpan sp{f.data(), size, a, end_bits, b == size, int64_t{1} << 30, 1 << 20};
        cs.pos = cur_abs - rel;
        int device_rc = 0;
        const int why = gz_chain_walk(sp, ch, res, cs, acc, [&](const GzChunk &c, GzResult *r) {
            *r = with_reach ? zlib_size_reach(f.data() + a, b - a, c.start, c.stop) : zlib_size(f.data() + a, b - a, c.start, c.stop);
            return 0;
        }, &device_rc);
        if (why) { std::printf("declined: %d (span %lld)\n", why, static_cast<long long>(spans)); return 1; }
        for (const GzAccepted &x : acc) {
            member += static_cast<uint64_t>(x.out_len);
            if (x.trailer >= 0) { got_len.push_back(member); member = 0; }
        }
        accepted += static_cast<int64_t>(acc.size());
        cur_abs = rel + cs.pos;
    }
    std::printf("spans %lld candidates %lld false_made %lld accepted %lld false_hits %lld rounds %lld members %lld\n", static_cast<long long>(spans),
                static_cast<long long>(found), static_cast<long long>(false_made), static_cast<long long>(accepted), static_cast<long long>(cs.false_hits),
                static_cast<long long>(cs.rounds), static_cast<long long>(cs.members));
    if (too_far_back) { std::printf("the chain accepted a file zlib refuses: invalid distance too far back\n"); return 1; }
    if (got_len != want_len) { std::printf("member lengths differ from zlib's\n"); return 1; }
    if (cs.false_hits != false_made) { std::printf("false hits: %lld made, %lld dropped\n", static_cast<long long>(false_made), static_cast<long long>(cs.false_hits)); return 1; }
    std::printf("chain ok\n");
    return 0;
}

struct Sink {
    palace_ctx *ctx;
    uint32_t crc = 0;
    uint64_t len = 0;
    bool last = false;
    std::vector<uint8_t> buf;
    static int take(void *user, const uint8_t *d_text, int64_t n, int last)
    {
        Sink *s = static_cast<Sink *>(user);
        s->buf.resize(static_cast<size_t>(n));
        if (n && palace_d2h(s->ctx, s->buf.data(), d_text, static_cast<size_t>(n))) return 1;
        for (int64_t p = 0; p < n; p += 1 << 30) s->crc = static_cast<uint32_t>(crc32(s->crc, s->buf.data() + p, static_cast<uInt>(std::min<int64_t>(1 << 30, n - p))));
        s->len += static_cast<uint64_t>(n);
        if (last) s->last = true;
        return 0;
    }
};

static int run_inflate(const std::vector<uint8_t> &f, int64_t stride, int64_t span)
{
    uint32_t want_crc = 0;
    uint64_t want_len = 0;
    bool zlib_ok = true;
    {
        z_stream zs{};
        inflateInit2(&zs, 31);
        std::vector<uint8_t> out(1 << 20);
        for (size_t pos = 0; pos < f.size() && zlib_ok;) {
            inflateReset(&zs);
            zs.next_in = const_cast<Bytef *>(f.data() + pos); zs.avail_in = static_cast<uInt>(f.size() - pos);
            int rc;
            do {
                zs.next_out = out.data(); zs.avail_out = static_cast<uInt>(out.size());
                rc = inflate(&zs, Z_NO_FLUSH);
                const size_t n = out.size() - zs.avail_out;
                want_crc = static_cast<uint32_t>(crc32(want_crc, out.data(), static_cast<uInt>(n)));
                want_len += n;
            } while (rc == Z_OK);
            zlib_ok = rc == Z_STREAM_END;
            pos = static_cast<size_t>(zs.next_in - f.data());
        }
        inflateEnd(&zs);
    }
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(0, &ctx)) { std::fprintf(stderr, "no device: %s\n", palace_last_error()); return 2; }
    Sink sink{ctx};
    palace_gzip_params prm{stride, span, 0, 0};
    palace_gzip_stats st;
    const int rc = palace_gzip_inflate(ctx, f.data(), static_cast<int64_t>(f.size()), &prm, &Sink::take, &sink, &st);
    palace_ctx_destroy(ctx);
    if (rc) { std::fprintf(stderr, "palace_gzip_inflate: %s\n", palace_last_error()); return 2; }
    std::printf("fallback %d found %lld accepted %lld false_hits %lld rounds %lld members %lld spans %lld batches %lld text %lld\n", st.fallback,
                static_cast<long long>(st.chunks_found), static_cast<long long>(st.chunks_accepted), static_cast<long long>(st.false_hits),
                static_cast<long long>(st.rounds), static_cast<long long>(st.members), static_cast<long long>(st.spans), static_cast<long long>(st.batches),
                static_cast<long long>(st.text_bytes));
    std::printf("ms: upload %.2f find %.2f size %.2f decode %.2f chain %.2f resolve %.2f crc %.2f sink %.2f\n", st.ms_upload, st.ms_find, st.ms_size,
                st.ms_decode, st.ms_chain, st.ms_resolve, st.ms_crc, st.ms_sink);
    if (st.fallback == 0 && !(zlib_ok && sink.last && sink.crc == want_crc && sink.len == want_len)) { std::printf("text differs from zlib's\n"); return 1; }
    if (st.fallback == 0) std::printf("text == zlib\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: gzip_selftest blocks|chain|inflate FILE [STRIDE SPAN [reach]]\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<uint8_t> f = read_file(argv[2]);
    const int64_t stride = argc > 3 ? std::atoll(argv[3]) : 0, span = argc > 4 ? std::atoll(argv[4]) : 0;
    if (mode == "blocks") {
        const std::vector<Block> b = block_starts(f);
        long dyn = 0;
        for (const Block &x : b) { std::printf("%lld %d %d\n", static_cast<long long>(x.bit), x.btype, x.bfinal); dyn += x.btype == 2 && !x.bfinal; }
        std::printf("blocks %zu dynamic_nonfinal %ld\n", b.size(), dyn);
        return 0;
    }
    if (mode == "chain") return run_chain(f, stride > 0 ? stride : 16384, span > 0 ? span : int64_t{64} << 20, argc > 5 && !std::strcmp(argv[5], "reach"));
    if (mode == "inflate") return run_inflate(f, stride, span);
    return 2;
}
