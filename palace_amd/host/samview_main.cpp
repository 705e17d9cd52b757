// samview -- the command between `bwa mem` and `samtools sort` that the driver gives to samtools (palace:421-423):
//     bwa mem ... | $SAMTOOLS view -@ "$threads" -F 0x0800 -buS - > tmp.bam
// as  bwa mem ... | samview -@ "$threads" -F 0x0800 -buS - > tmp.bam        (the argument list as the driver has it)
// The SAM text goes up once; its lines are found, validated, filtered and encoded as BAM records on the device (sam_device.hpp,
// csrc/sam.hip), the stream is cut into members of 0xff00 bytes -- stored ones with -u, the host framing what the device has summed;
// the device coder's otherwise (bgzf_members_device.hpp; --lz: the coder for text without lines, palace_bgzf_deflate_lz) -- and the EOF member ends the file.  The host parses the header and the
// command line, nothing else.  The rules are DESIGN.md 8; htslib is not at hand, so parity with samtools is UNPINNED.
// Needs a device: there is no host path behind it.  On any failure no output file is left and nothing has gone to stdout.
//   PALACE_DEVICE, PALACE_TRACE      as in the other tools
#include <iostream>

#include "bai.hpp"
#include "bgzf_members_device.hpp"
#include "device_pick.hpp"
#include "sam_device.hpp"

using namespace palace_host;

namespace {

int usage()
{
    std::cerr << "Usage: samview [-@ <threads>] [-F <mask>] -b [-u | --lz] [-S] [-h] [-o <out.bam>] <in.sam | ->\n"
              << "  SAM text to BAM; -F: drop the lines whose FLAG has a bit of <mask> (decimal or 0x hex); -u: stored (uncompressed) members;\n"
              << "  --lz: members with hashed matches (smaller files; not with -u);\n"
              << "  -b is required (only BAM is written); -S, -h and -@ are accepted and ignored; short flags may be clustered (-buS);\n"
              << "  output goes to -o or stdout.  Tags of type f and B:f are refused (no text-to-float on the device; bwa writes none).\n"
              << "  no other option of `samtools view` is taken; parity with samtools is unpinned (DESIGN.md 8)\n";
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<std::string> a(argv + 1, argv + argc);
    std::string in, out;
    bool have_in = false, bam = false, stored = false, lz = false;
    uint32_t mask = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const std::string &s = a[i];
        if (s == "-" || s.empty() || s[0] != '-') {
            if (have_in) return usage();
            in = s; have_in = true;
            continue;
        }
        if (s == "--lz") { lz = true; continue; }
        for (size_t k = 1; k < s.size(); k++) {
            const char c = s[k];
            if (c == 'b') bam = true;
            else if (c == 'u') stored = true;
            else if (c == 'S' || c == 'h') continue;
            else if (c == '@' || c == 'F' || c == 'o') {                     // the value: the rest of the word, or the next word
                std::string v;
                if (k + 1 < s.size()) v = s.substr(k + 1);
                else if (i + 1 < a.size()) v = a[++i];
                else return usage();
                if (c == '@' && (v.empty() || v.size() > 6 || v.find_first_not_of("0123456789") != std::string::npos)) return usage();
                if (c == 'F' && !parse_flag_mask(v, &mask)) return usage();
                if (c == 'o') { if (v.empty()) return usage(); out = v; }
                break;
            } else return usage();
        }
    }
    if (!have_in || in.empty() || (lz && stored)) return usage();
    if (!bam) { std::cerr << "samview: only BAM is written: -b is required\n"; return 1; }

    return with_device("samview", [&](palace_ctx *ctx) {
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;
        StageClock clock{ctx, trace};
        MemberWriteTimes wt;
        SamTimes tm;
        DeviceBamStream st;
        int64_t dropped = 0;
        load_sam_stream_device(ctx, in, mask, st, trace ? &tm : nullptr, &dropped);      // (the whole conversion: nothing is written before it is done)
        const std::string out_name = out.empty() ? "stdout" : out;
        OutputFiles outputs;                                                 // (stdout is not its to close or remove)
        FILE *f = out.empty() ? stdout : (outputs.f = std::fopen(out.c_str(), "wb"));
        if (!f) throw std::runtime_error("cannot open " + out + " for writing");
        if (!out.empty()) outputs.made.push_back(out);
        std::vector<int64_t> member_u, member_c;
        uint64_t file_bytes = 0;
        write_bam_file_device(ctx, bamsort_no_room, st.d_stream, st.total, 8192, stored, lz, f, out_name, clock, wt, member_u, member_c, &file_bytes);
        const int rc_close = out.empty() ? std::fflush(f) : std::fclose(f);
        outputs.f = nullptr;
        if (rc_close != 0) throw std::runtime_error("write failed: " + out_name);
        outputs.done = true;
        if (trace)
            std::fprintf(stderr, "[samview] ms: read %.1f upload %.1f lines %.1f plan %.1f encode %.1f | crc%s %.1f copy+write %.1f; records %lld, dropped %lld, "
                         "stream %lld B, file %llu B\n", tm.read, tm.upload, tm.lines, tm.plan, tm.encode, stored ? "" : "+deflate", wt.crc + wt.deflate, wt.copy_write,
                         static_cast<long long>(st.n_records), static_cast<long long>(dropped), static_cast<long long>(st.total),
                         static_cast<unsigned long long>(file_bytes));
        return 0;
    });
}
