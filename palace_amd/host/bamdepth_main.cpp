// bamdepth -- the mean depth the driver computes before generateGraph (palace:538-552):
//     samtools depth -@ T <bam> > <bam>.depth ; first_depth=$(awk '{sum+=$3} END { print sum/NR }' <bam>.depth)
// as one command:   first_depth=$(bamdepth <bam>)
// prints exactly what the awk line prints.
//     bamdepth --per-contig <bam> > contig_depth.tsv
// prints `contig <TAB> depth sum <TAB> covered positions` for every contig with coverage: the two numbers step 5 takes from
// the tabix-indexed depth file per contig (create_sub_graph.py:186-234); palace_amd/scripts/create_sub_graph.py reads it.
//     first_depth=$(bamdepth --depth-gz <bam>.depth.gz <bam>)
// writes the per-base depth file itself -- <bam>.depth.gz (the text of `samtools depth`, BGZF) and <bam>.depth.gz.tbi (the index
// `tabix -s 1 -b 2 -e 2` makes) -- and prints the awk number: the four commands of palace:541-545 as one, host only (depthgz.hpp).
//     first_depth=$(bamdepth --depth-gz-gpu <bam>.depth.gz <bam>)
// writes the same two files with the text, its CRC-32, the DEFLATE members and the index's offsets computed on the device
// (depthgz_device.hpp): same text, same cut into members, same index once virtual offsets are mapped to text offsets; the
// compressed bytes are the device coder's.  Opt-in; without a device it fails like `bamdepth <bam>`, it does not fall back.
//     first_depth=$(bamdepth --bam-gpu [--per-contig | --depth-gz-gpu <bam>.depth.gz] <bam>)
// prints (and writes) the same with the BAM itself read on the device (bam_stream_device.hpp): its BGZF members are inflated and
// CRC-checked there, the record starts found (palace_bam_walk) and the match segments made (palace_bam_match_segments) where the
// inflated stream lies, and handed to the depth kernels as device pointers; the host parses the header only.  With --depth-gz-gpu
// the stage is file -> device -> file.  `--bam-gpu` comes first; `--bam-gpu --depth-gz` is a usage error (that mode is host only).
// Opt-in; the whole inflated BAM must fit the device; without a device it fails like `bamdepth <bam>`, it never falls back to
// the host loader.  PALACE_TRACE prints the loader's laps and the walk's statistics.
//     first_depth=$(bamdepth --from-depth <bam>.depth.gz)        bamdepth --from-depth --per-contig <bam>.depth.gz > contig_depth.tsv
// print the same two things from the depth file itself (depth_read.hpp): plain text or BGZF, told apart by the first bytes; BGZF
// members are inflated and CRC-checked on the device, the text is parsed there (palace_depth_parse) and never comes to the host.
// `--from-depth` comes first and goes with no other mode.  Opt-in; without a device it fails, there is no host parser behind it.
// PALACE_TRACE prints the laps.
// (`generateGraph <bam> <fai> <out> auto` uses the same number without a second pass over the BAM.)
#include <algorithm>
#include <iostream>
#include <thread>

#include "bam.hpp"
#include "bam_stream_device.hpp"
#include "device_pick.hpp"
#include "depth_host.hpp"
#include "depth_read.hpp"
#include "depthgz.hpp"
#include "depthgz_device.hpp"

using namespace palace_host;

// the awk number on stdout, or awk's complaint (exit code 2)
static int print_mean(uint64_t sum, uint64_t lines)
{
    if (lines == 0) { std::cerr << "bamdepth: no position is covered (awk: division by zero)\n"; return 2; }
    std::cout << awk_number(static_cast<double>(sum) / static_cast<double>(lines)) << "\n";
    return 0;
}

// `contig <TAB> depth sum <TAB> covered positions` for every contig with coverage
static int print_per_contig(const std::vector<std::string> &name, const std::vector<uint64_t> &sum, const std::vector<uint64_t> &covered)
{
    std::string out;
    for (size_t t = 0; t < sum.size(); t++)
        if (covered[t]) out += name[t] + "\t" + std::to_string(sum[t]) + "\t" + std::to_string(covered[t]) + "\n";
    std::cout << out;
    return 0;
}

// --depth-gz-gpu: what the writer reports (traced runs), then the mean
static int report_depth_gz_gpu(const DepthGzResult &r, const DepthGzDeviceTimes &tm, bool trace)
{
    if (trace)
        std::fprintf(stderr, "[bamdepth] depth-gz-gpu ms: upload %.1f create %.1f emit %.1f crc %.1f deflate+compact %.1f d2h+write %.1f windows %.1f tbi %.1f; "
                     "text %llu B, file %llu B\n", tm.upload, tm.create, tm.members.emit, tm.members.crc, tm.members.deflate, tm.members.copy_write, tm.windows, tm.tbi,
                     static_cast<unsigned long long>(r.text_bytes), static_cast<unsigned long long>(r.file_bytes));
    return print_mean(r.sum, r.lines);
}

// the mean or the per-contig table from first_depth's answer
static int print_first_depth(int rc, bool per_contig, const std::string &text, const std::vector<std::string> &name, const std::vector<uint64_t> &cs,
                             const std::vector<uint64_t> &cc)
{
    if (rc < 0) throw std::runtime_error(palace_last_error());
    if (per_contig) return print_per_contig(name, cs, cc);
    if (rc > 0) return print_mean(0, 0);
    std::cout << text << "\n";
    return 0;
}

// `bamdepth --bam-gpu ...`: argv[1 ..] are the arguments behind --bam-gpu, parsed as main() parses them
static int main_bam_gpu(bool per_contig, bool depth_gz_gpu, const char *gz_path, const char *bam, int threads)
{
    return with_device("bamdepth", [&](palace_ctx *ctx) {
        DeviceBam b;
        BamDeviceTimes bt;
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;
        try {
            load_bam_device(ctx, bam, threads, b, trace ? &bt : nullptr);
        } catch (const std::exception &e) { throw std::runtime_error(std::string(bam) + ": " + e.what()); }
        if (trace)
            std::fprintf(stderr, "[bamdepth] bam-gpu ms: member index %.1f header %.1f upload %.1f inflate %.1f crc %.1f walk %.1f segments %.1f; "
                         "walk: chunks %lld, guesses held %lld, repaired %lld, without a start %lld; stream %lld B, records %lld, segments %lld, "
                         "members inflated on the host %lld\n", bt.index, bt.header, bt.upload, bt.inflate, bt.crc, bt.walk, bt.segments,
                         static_cast<long long>(b.walk_stats[0]), static_cast<long long>(b.walk_stats[1]), static_cast<long long>(b.walk_stats[2]),
                         static_cast<long long>(b.walk_stats[3]), static_cast<long long>(b.total), static_cast<long long>(b.n_records),
                         static_cast<long long>(b.n_segs), static_cast<long long>(b.host_inflated));
        if (depth_gz_gpu) {
            DepthGzDeviceTimes tm;
            const DepthGzResult r = write_depth_gz_device(ctx, b.n_segs, b.d_tid, b.d_pos, b.d_len, b.target_name, b.target_len, gz_path, trace ? &tm : nullptr);
            return report_depth_gz_gpu(r, tm, trace);
        }
        std::string text;
        std::vector<uint64_t> cs, cc;
        const int rc = per_contig ? first_depth(ctx, b.n_segs, b.d_tid, b.d_pos, b.d_len, b.target_len, text, nullptr, nullptr, &cs, &cc)
                                  : first_depth(ctx, b.n_segs, b.d_tid, b.d_pos, b.d_len, b.target_len, text);
        return print_first_depth(rc, per_contig, text, b.target_name, cs, cc);
    });
}

// `bamdepth --from-depth [--per-contig] <depth file>`
static int main_from_depth(bool per_contig, const char *file)
{
    return with_device("bamdepth", [&](palace_ctx *ctx) {
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;
        DepthReadTimes tm;
        const DepthReadResult r = read_depth_file(ctx, file, trace ? &tm : nullptr);
        if (trace)
            std::fprintf(stderr, "[bamdepth] from-depth ms: index %.1f upload %.1f inflate %.1f crc %.1f parse %.1f merge %.1f; text %llu B, lines %llu, "
                         "runs %llu, members inflated on the host %llu\n", tm.index, tm.upload, tm.inflate, tm.crc, tm.parse, tm.merge,
                         static_cast<unsigned long long>(r.text_bytes), static_cast<unsigned long long>(r.lines), static_cast<unsigned long long>(r.runs),
                         static_cast<unsigned long long>(r.host_inflated));
        if (!per_contig) return print_mean(r.sum, r.lines);
        std::string out;                                                     // (every contig of the file has lines)
        for (size_t t = 0; t < r.name.size(); t++) out += r.name[t] + "\t" + std::to_string(r.contig_sum[t]) + "\t" + std::to_string(r.contig_lines[t]) + "\n";
        std::cout << out;
        return 0;
    });
}

static int usage(const char *prog)
{
    std::cerr << "Usage: " << prog << " [--bam-gpu] [--per-contig | --depth-gz <out.depth.gz> | --depth-gz-gpu <out.depth.gz>] <bam>"
              << "   (--bam-gpu: the BAM is read on the device; not with --depth-gz, the host-only mode)"
              << "  |  " << prog << " --from-depth [--per-contig] <depth file>   (the depth file, plain or BGZF, read back on the device)\n";
    return 1;
}

int main(int argc, char **argv)
{
    const char *prog = argv[0];
    if (argc >= 2 && std::string(argv[1]) == "--from-depth") {       // its own command line: [--per-contig] <depth file>, nothing else
        const bool pc = argc >= 3 && std::string(argv[2]) == "--per-contig";
        if (argc != (pc ? 4 : 3) || std::string(argv[argc - 1]).rfind("--", 0) == 0) return usage(prog);
        return main_from_depth(pc, argv[argc - 1]);
    }
    const bool bam_gpu = argc >= 2 && std::string(argv[1]) == "--bam-gpu";
    if (bam_gpu) { argc--; argv++; }                 // the rest is parsed as without it
    const bool per_contig = argc >= 3 && std::string(argv[1]) == "--per-contig";
    const bool gz_mode = argc >= 2 && (std::string(argv[1]) == "--depth-gz" || std::string(argv[1]) == "--depth-gz-gpu");
    const bool depth_gz_gpu = argc >= 4 && std::string(argv[1]) == "--depth-gz-gpu";
    const bool depth_gz = argc >= 4 && gz_mode;
    if (argc < 2 || (per_contig && argc < 3) || (gz_mode && argc < 4) || (bam_gpu && depth_gz && !depth_gz_gpu)) {
        return usage(prog);
    }
    const char *bam = depth_gz ? argv[3] : per_contig ? argv[2] : argv[1];
    const int threads = static_cast<int>(std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    if (bam_gpu) return main_bam_gpu(per_contig, depth_gz_gpu, depth_gz_gpu ? argv[2] : nullptr, bam, threads);
    BamColumns c;
    try {
        load_bam(bam, threads, 1, c);
    } catch (const std::exception &e) { std::cerr << e.what() << "\n"; return 1; }
    if (depth_gz_gpu)                                // text, CRC-32, DEFLATE and the index's offsets on the device
        return with_device("bamdepth", [&](palace_ctx *ctx) {
            DepthGzDeviceTimes tm;
            const bool trace = std::getenv("PALACE_TRACE") != nullptr;
            return report_depth_gz_gpu(write_depth_gz_device(ctx, c, argv[2], trace ? &tm : nullptr), tm, trace);
        });
    if (depth_gz) {                                  // no GPU in this mode: text and DEFLATE are host work
        try {
            const DepthGzResult r = write_depth_gz(c, argv[2], threads);
            return print_mean(r.sum, r.lines);
        } catch (const std::exception &e) { std::cerr << "bamdepth: " << e.what() << "\n"; return 1; }
    }
    return with_device("bamdepth", [&](palace_ctx *ctx) {
        std::string text;
        std::vector<uint64_t> cs, cc;
        const int rc = per_contig ? first_depth(ctx, c, text, nullptr, nullptr, &cs, &cc) : first_depth(ctx, c, text);
        return print_first_depth(rc, per_contig, text, c.target_name, cs, cc);
    });
}
