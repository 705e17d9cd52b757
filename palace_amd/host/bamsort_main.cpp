// bamsort -- the two commands between `bwa` and generateGraph that the driver gives to samtools (palace:425-433):
//     $SAMTOOLS sort -@ "$threads" tmp.bam -O BAM -o first_bam ; $SAMTOOLS index first_bam
// as   bamsort -@ "$threads" tmp.bam -O BAM -o first_bam --bai      (the argument list of `samtools sort`, in any order, + --bai)
// or   bamsort ... -o first_bam ; bamsort --index first_bam [<out.bai>]
// or   bwa mem ... | bamsort --sam -F 0x0800 -@ "$threads" - -O BAM -o first_bam --bai     (palace:421-433 as one command: the input is
//      bwa's SAM text, encoded on the device as `samview` does it (sam_device.hpp), and tmp.bam never exists)
// The BAM is inflated, CRC-checked and walked on the device (bam_stream_device.hpp), its records are keyed (palace_bam_sort_keys),
// the keys sorted with a stable radix sort (palace_sort_u64), the records gathered behind the rewritten header
// (palace_bam_gather_plan / _write), the stream cut into members of 0xff00 bytes that the device coder deflates (palace_crc32_members,
// palace_bgzf_deflate, palace_bgzf_compact; bgzf_members_device.hpp), and the .bai computed from the stream that was
// written (bai.hpp).  The host rewrites the header and lays out the index, nothing else.  The rules are DESIGN.md 8.
// Needs a device: there is no host path behind it.  On any failure no output file is left.
//   --lz                             the members come from the coder for text without lines (palace_bgzf_deflate_lz: hashed matches)
//   -@ <n>                           host threads that inflate the header's members; otherwise ignored
//   PALACE_DEVICE, PALACE_TRACE      as in the other tools
//   PALACE_OPT_BAMSORT_BATCH=<n>     members per deflate batch (tests); PALACE_OPT_BAM_BATCH / PALACE_OPT_BAM_CHUNK on the input side
#include <iostream>

#include "bai.hpp"
#include "bam_stream_device.hpp"
#include "bgzf_members_device.hpp"
#include "device_pick.hpp"
#include "sam_device.hpp"

using namespace palace_host;

namespace {

int usage()
{
    std::cerr << "Usage: bamsort [-@ <threads>] [-O BAM] -o <out.bam> [--bai] [--lz] <in.bam>   (coordinate sort; --bai also writes <out.bam>.bai;\n"
              << "                                                                            --lz: members with hashed matches, smaller files)\n"
              << "       bamsort --sam [-F <mask>] ... -o <out.bam> [--bai] [--lz] <in.sam | ->     (the input is SAM text, as samview takes it)\n"
              << "       bamsort --index <sorted.bam> [<out.bai>]                       (default <sorted.bam>.bai)\n"
              << "no other option of `samtools sort` / `samtools index` is taken\n";
    return 1;
}

// members per deflate batch: 8192, as the depth file's writer; PALACE_OPT_BAMSORT_BATCH=<members> for tests
size_t bamsort_batch_members()
{
    const char *e = std::getenv("PALACE_OPT_BAMSORT_BATCH");
    const long v = e ? std::atol(e) : 0;
    return v > 0 ? static_cast<size_t>(std::min<long>(v, 8192)) : 8192;
}

int bits_of(uint32_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

// The header [0, first) of the input stream as the output's: the text's @HD line says SO:coordinate, nothing else changes.
std::vector<uint8_t> rewrite_header(const std::vector<uint8_t> &in)
{
    uint32_t l_text;
    std::memcpy(&l_text, in.data() + 4, 4);
    std::string text(reinterpret_cast<const char *>(in.data()) + 8, l_text);
    if (text.rfind("@HD\t", 0) == 0) {
        const size_t eol = std::min(text.find('\n'), text.size());
        size_t so = std::string::npos;
        for (size_t f = 3; f < eol;) {                                       // text[f] is the TAB in front of a field
            const size_t b = f + 1, e = std::min(text.find('\t', b), eol);
            if (e - b >= 3 && text.compare(b, 3, "SO:") == 0) { so = b; break; }
            f = e;
        }
        if (so == std::string::npos) text.insert(eol, "\tSO:coordinate");
        else text.replace(so + 3, std::min(text.find('\t', so), eol) - (so + 3), "coordinate");
    } else
        text.insert(0, "@HD\tVN:1.6\tSO:coordinate\n");
    std::vector<uint8_t> out(in.begin(), in.begin() + 4);
    const uint32_t n = static_cast<uint32_t>(text.size());
    for (int k = 0; k < 4; k++) out.push_back(static_cast<uint8_t>(n >> (8 * k)));
    out.insert(out.end(), text.begin(), text.end());
    out.insert(out.end(), in.begin() + 8 + l_text, in.end());
    return out;
}

// laps of a traced run
struct Laps { double keys = 0, sort = 0, gather = 0, index = 0; MemberWriteTimes write; };

// the loader's errors name the input; an out-of-room message stands alone
template <class Load> void load_named(const std::string &in, Load load)
{
    try {
        load();
    } catch (const DeviceNoRoom &) { throw;
    } catch (const std::exception &e) { throw std::runtime_error(in + ": " + e.what()); }
}

void require_whole(const DeviceBamStream &st)
{
    if (st.stop != st.total) throw std::runtime_error("malformed record at offset " + std::to_string(st.stop) + " (the stream has " + std::to_string(st.total) + " bytes)");
    if (st.n_records > 0x7fffffffll) throw std::runtime_error("more than 2^31 - 1 records");
}

int main_sort(const std::string &in, const std::string &out, bool bai, int threads, bool sam, uint32_t mask, bool lz)
{
    return with_device("bamsort", [&](palace_ctx *ctx) {
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;
        StageClock clock{ctx, trace};
        Laps laps;
        BamDeviceTimes bt;
        SamTimes sam_tm;
        DeviceBamStream st;
        load_named(in, [&] {
            if (sam) load_sam_stream_device(ctx, in, mask, st, trace ? &sam_tm : nullptr);
            else load_bam_stream_device(ctx, in, threads, st, trace ? &bt : nullptr);
            require_whole(st);
        });
        const size_t n = static_cast<size_t>(st.n_records);
        DeviceScope dev(ctx, bamsort_no_room);

        // the header: the one part the host touches
        std::vector<uint8_t> head(static_cast<size_t>(st.first));
        ck(palace_d2h(ctx, head.data(), st.d_stream, head.size()), "palace_d2h");
        const std::vector<uint8_t> new_head = rewrite_header(head);

        clock.restart();
        uint64_t *d_key = dev.array<uint64_t>(n, "the sort keys");
        int64_t n_bad = 0, first_bad = -1;
        ck(palace_bam_sort_keys(ctx, st.d_stream, st.total, st.d_starts, st.n_records, st.n_ref, d_key, &n_bad, &first_bad), "palace_bam_sort_keys");
        if (n_bad)
            throw std::runtime_error(in + ": record " + std::to_string(first_bad) + ": refID or pos outside what the header's " + std::to_string(st.n_ref) +
                                     " targets allow (" + std::to_string(n_bad) + " such records)");
        clock.lap(&laps.keys, true);
        uint32_t *d_perm = dev.array<uint32_t>(n, "the permutation");
        const size_t sort_bytes = palace_sort_u64_scratch_bytes(st.n_records);
        void *d_sort = dev.alloc(sort_bytes, "the sort's scratch");
        ck(palace_sort_u64(ctx, d_key, d_perm, st.n_records, 33 + bits_of(static_cast<uint32_t>(st.n_ref)), d_sort, sort_bytes), "palace_sort_u64");
        ck(palace_sync(ctx), "palace_sync");
        clock.lap(&laps.sort, true);
        dev.give_back(d_sort);
        dev.give_back(d_key);

        int64_t *d_out_off = dev.array<int64_t>(n + 1, "the output offsets");
        int64_t *d_out_starts = bai ? dev.array<int64_t>(n, "the output's record starts") : nullptr;
        int64_t out_bytes = 0;
        ck(palace_bam_gather_plan(ctx, st.d_stream, st.d_starts, d_perm, st.n_records, static_cast<int64_t>(new_head.size()), d_out_off, d_out_starts, &out_bytes),
           "palace_bam_gather_plan");
        uint8_t *d_out = dev.array<uint8_t>(static_cast<size_t>(out_bytes) + 64, "the sorted stream");
        ck(palace_h2d(ctx, d_out, new_head.data(), new_head.size()), "palace_h2d");
        ck(palace_bam_gather_write(ctx, st.d_stream, st.d_starts, d_perm, d_out_off, st.n_records, out_bytes, d_out), "palace_bam_gather_write");
        ck(palace_sync(ctx), "palace_sync");
        clock.lap(&laps.gather, true);
        st.release();                                                        // the input has been copied
        dev.give_back(d_perm);
        dev.give_back(d_out_off);

        // the file: members of 0xff00 bytes, a batch at a time
        std::vector<int64_t> member_u, member_c;
        uint64_t file_bytes = 0;
        OutputFiles outputs;
        outputs.f = std::fopen(out.c_str(), "wb");
        if (!outputs.f) throw std::runtime_error("cannot open " + out + " for writing");
        outputs.made.push_back(out);
        write_bam_file_device(ctx, bamsort_no_room, d_out, out_bytes, bamsort_batch_members(), false, lz, outputs.f, out, clock, laps.write, member_u, member_c, &file_bytes);
        const int rc_close = std::fclose(outputs.f);
        outputs.f = nullptr;
        if (rc_close != 0) throw std::runtime_error("write failed: " + out);
        clock.lap(&laps.write.copy_write, true);

        if (bai) {
            clock.restart();
            outputs.made.push_back(out + ".bai");
            write_bai_device(ctx, out, d_out, d_out_starts, st.n_records, st.n_ref, member_u, member_c, out + ".bai");
            clock.lap(&laps.index, true);
        }
        outputs.done = true;
        if (trace && sam)
            std::fprintf(stderr, "[bamsort] --sam ms: read %.1f upload %.1f lines %.1f plan %.1f encode %.1f\n", sam_tm.read, sam_tm.upload, sam_tm.lines, sam_tm.plan,
                         sam_tm.encode);
        if (trace)
            std::fprintf(stderr, "[bamsort] ms: member index %.1f header %.1f upload %.1f inflate %.1f crc %.1f walk %.1f | keys %.1f sort %.1f gather %.1f "
                         "crc+deflate %.1f copy+write %.1f index %.1f; records %lld, stream %lld B -> %lld B, file %llu B, members inflated on the host %lld\n",
                         bt.index, bt.header, bt.upload, bt.inflate, bt.crc, bt.walk, laps.keys, laps.sort, laps.gather, laps.write.crc + laps.write.deflate,
                         laps.write.copy_write, laps.index, static_cast<long long>(st.n_records), static_cast<long long>(st.total), static_cast<long long>(out_bytes),
                         static_cast<unsigned long long>(file_bytes), static_cast<long long>(st.host_inflated));
        return 0;
    });
}

int main_index(const std::string &bam, const std::string &bai_path, int threads)
{
    return with_device("bamsort", [&](palace_ctx *ctx) {
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;
        StageClock clock{ctx, trace};
        double index_ms = 0;
        BamDeviceTimes bt;
        DeviceBamStream st;
        BamMemberTable members;                                              // the file's own member table (the loader has checked it)
        load_named(bam, [&] {
            load_bam_stream_device(ctx, bam, threads, st, trace ? &bt : nullptr, {}, &members);
            require_whole(st);
        });
        clock.restart();
        write_bai_device(ctx, bam, st.d_stream, st.d_starts, st.n_records, st.n_ref, members.u, members.c, bai_path);
        clock.lap(&index_ms, true);
        if (trace)
            std::fprintf(stderr, "[bamsort] index ms: member index %.1f header %.1f upload %.1f inflate %.1f crc %.1f walk %.1f | index %.1f; records %lld, stream %lld B\n",
                         bt.index, bt.header, bt.upload, bt.inflate, bt.crc, bt.walk, index_ms, static_cast<long long>(st.n_records), static_cast<long long>(st.total));
        return 0;
    });
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<std::string> a(argv + 1, argv + argc);
    int threads = 1;
    if (std::find(a.begin(), a.end(), "--index") != a.end()) {
        std::vector<std::string> pos;
        for (const std::string &s : a) {
            if (s == "--index") continue;
            if (s.size() > 1 && s[0] == '-') return usage();
            pos.push_back(s);
        }
        if (pos.empty() || pos.size() > 2) return usage();
        return main_index(pos[0], pos.size() == 2 ? pos[1] : pos[0] + ".bai", 16);
    }
    std::string in, out, fmt = "BAM";
    bool bai = false, have_in = false, sam = false, have_mask = false, lz = false;
    uint32_t mask = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const std::string &s = a[i];
        auto value = [&](std::string *v) {                                   // `-x value` or `-xvalue`
            if (s.size() > 2) { *v = s.substr(2); return true; }
            if (i + 1 >= a.size()) return false;
            *v = a[++i];
            return true;
        };
        if (s == "--bai") bai = true;
        else if (s == "--sam") sam = true;
        else if (s == "--lz") lz = true;
        else if (s == "-" && !have_in) { in = s; have_in = true; }
        else if (s.rfind("-F", 0) == 0) {
            std::string v;
            if (!value(&v) || !parse_flag_mask(v, &mask)) return usage();
            have_mask = true;
        } else if (s.rfind("-@", 0) == 0) {
            std::string v;
            if (!value(&v) || v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 6) return usage();
            threads = std::max(1, std::atoi(v.c_str()));
        } else if (s.rfind("-O", 0) == 0) {
            if (!value(&fmt)) return usage();
        } else if (s.rfind("-o", 0) == 0) {
            if (!value(&out) || out.empty()) return usage();
        } else if (s.size() > 1 && s[0] == '-') return usage();
        else if (have_in) return usage();
        else { in = s; have_in = true; }
    }
    if (!have_in || out.empty() || (!sam && (have_mask || in == "-"))) return usage();
    if (fmt != "BAM" && fmt != "bam") { std::cerr << "bamsort: -O " << fmt << ": only BAM is written\n"; return 1; }
    return main_sort(in, out, bai, std::min(threads, 64), sam, mask, lz);
}
