// The front end `samview` and `bamsort --sam` share: a SAM text becomes a DeviceBamStream -- the BAM stream (header and records) and
// the records' starts in device memory, as load_bam_stream_device leaves them for a BAM file -- without a BAM ever being written.
// The text is read whole (a file, or stdin for `-`) and goes up once; the header is parsed here (sam_header.hpp), everything else
// on the device: palace_sam_lines, palace_sam_plan, palace_sam_encode (csrc/sam.hip; the rules: DESIGN.md 8, csrc/sam_line.hpp).
// Nothing is written anywhere before the whole text has been validated.  Device memory held at once: the text, the stream, 24 bytes
// per line and 8 per record.  No host path: a text that does not fit is refused.
#pragma once
#include <cstdio>

#include "bam_stream_device.hpp"
#include "sam_header.hpp"

namespace palace_host {

struct SamTimes { double read = 0, upload = 0, lines = 0, plan = 0, encode = 0; };

// a grammar error: what() is `line N: <reason>`
struct SamError : std::runtime_error {
    SamError(int64_t line, int code) : std::runtime_error("line " + std::to_string(line) + ": " + sam_error_text(code)) {}
};
// the out-of-room text of the SAM front end
inline std::string sam_no_room(size_t bytes, const char *what, const char *err)
{
    return "the SAM text, the BAM stream, 24 bytes per line and 8 per record are kept on the device, and " + std::to_string(bytes) + " bytes for " + what +
           " cannot be allocated (" + err + "); there is no host path, a text larger than device memory is out of scope";
}

// `-F`'s value: decimal or 0x hex, nothing else
inline bool parse_flag_mask(const std::string &v, uint32_t *mask)
{
    const bool hex = v.size() > 2 && v[0] == '0' && (v[1] == 'x' || v[1] == 'X');
    const std::string digits = hex ? v.substr(2) : v;
    if (digits.empty() || digits.size() > 8 || digits.find_first_not_of(hex ? "0123456789abcdefABCDEF" : "0123456789") != std::string::npos) return false;
    const unsigned long x = std::strtoul(digits.c_str(), nullptr, hex ? 16 : 10);
    if (x > 0xffff) return false;
    *mask = static_cast<uint32_t>(x);
    return true;
}

inline std::vector<uint8_t> read_whole(const std::string &path)
{
    FILE *f = path == "-" ? stdin : std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<uint8_t> text;
    std::vector<uint8_t> buf(1u << 20);
    for (size_t got; (got = std::fread(buf.data(), 1, buf.size(), f)) > 0;) text.insert(text.end(), buf.begin(), buf.begin() + static_cast<std::ptrdiff_t>(got));
    const bool bad = std::ferror(f) != 0;
    if (f != stdin) std::fclose(f);
    if (bad) throw std::runtime_error("cannot read " + path);
    return text;
}

inline void load_sam_stream_device(palace_ctx *ctx, const std::string &path, uint32_t mask, DeviceBamStream &out, SamTimes *times = nullptr,
                                   int64_t *n_dropped_out = nullptr)
{
    SamTimes unused;
    SamTimes &tm = times ? *times : unused;
    StageClock clock{ctx, times != nullptr};
    DeviceScope own(ctx, sam_no_room);

    const std::vector<uint8_t> text = read_whole(path);
    const int64_t n = static_cast<int64_t>(text.size());
    const SamHeader hdr = parse_sam_header(text.data(), text.size());
    if (hdr.code) throw SamError(hdr.line, hdr.code);
    if (hdr.name.size() > 0x7fffffffu || hdr.text_bytes > 0x7fffffffu) throw std::runtime_error("the header is too large for a BAM");
    const std::vector<uint8_t> head = bam_header_bytes(hdr, text.data());
    clock.lap(&tm.read, false);

    uint8_t *d_text = static_cast<uint8_t *>(own.alloc(static_cast<size_t>(n) + 64, "the text"));
    if (n) ck(palace_h2d(ctx, d_text, text.data(), text.size()), "text upload");
    clock.lap(&tm.upload, true);

    // the lines: counted first, then written into exactly that much memory
    const size_t scratch_bytes = palace_sam_scratch_bytes(n);
    void *d_scratch = own.alloc(scratch_bytes, "the line count");
    int64_t res[5];
    ck(palace_sam_lines(ctx, d_text, n, d_scratch, scratch_bytes, nullptr, 0, res), "palace_sam_lines");
    const int64_t n_lines = res[0];
    int64_t *d_line = static_cast<int64_t *>(own.alloc(static_cast<size_t>(n_lines + 1) * 8, "the line starts"));
    ck(palace_sam_lines(ctx, d_text, n, d_scratch, scratch_bytes, d_line, n_lines + 1, res), "palace_sam_lines");
    const int64_t lines_err_line = res[3];
    const int lines_err_code = static_cast<int>(res[4]);
    if (res[1] != hdr.n_lines) throw std::runtime_error("palace_sam_lines: the header has " + std::to_string(hdr.n_lines) + " lines, the device counts " + std::to_string(res[1]));
    // an empty line or a late '@' line: the lines in front of it are still validated, the smallest faulty line is the one reported
    const int64_t n_header = res[1], n_align = lines_err_code ? lines_err_line - 1 - res[1] : res[2];
    if (n_align > 0x7fffffffll) throw std::runtime_error("more than 2^31 - 1 records");
    clock.lap(&tm.lines, true);

    // the header's names for RNAME / RNEXT: one blob, offsets, the table built from them on the device
    const DeviceNames names = upload_names(own, hdr.name, "the target names", "target names");
    BamNamesHandle table_guard(ctx);
    ck(palace_bam_names_create(ctx, names.blob, names.off, static_cast<int32_t>(hdr.name.size()), &table_guard.h), "palace_bam_names_create");
    palace_bam_names *const table = table_guard.h;

    const size_t na = static_cast<size_t>(n_align);
    int32_t *d_size = static_cast<int32_t *>(own.alloc(na * 4, "the record sizes"));
    int64_t *d_off = static_cast<int64_t *>(own.alloc((na + 1) * 8, "the record offsets"));
    int32_t *d_ord = static_cast<int32_t *>(own.alloc(na * 4, "the record ordinals"));
    ck(palace_sam_plan(ctx, d_text, d_line + n_header, n_align, n_header + 1, table, mask, static_cast<int64_t>(head.size()), d_size, d_off, d_ord, res), "palace_sam_plan");
    if (res[4]) throw SamError(res[3], static_cast<int>(res[4]));
    if (lines_err_code) throw SamError(lines_err_line, lines_err_code);
    const int64_t kept = res[0], total = res[2];
    clock.lap(&tm.plan, true);

    uint8_t *d_stream = static_cast<uint8_t *>(own.alloc(static_cast<size_t>(total) + 64, "the BAM stream"));
    int64_t *d_starts = static_cast<int64_t *>(own.alloc(static_cast<size_t>(kept) * 8, "the record starts"));
    ck(palace_h2d(ctx, d_stream, head.data(), head.size()), "header upload");
    ck(palace_sam_encode(ctx, d_text, d_line + n_header, n_align, table, d_size, d_off, d_ord, d_stream, d_starts), "palace_sam_encode");
    ck(palace_sync(ctx), "palace_sync");
    clock.lap(&tm.encode, true);

    own.keep(d_stream);
    own.keep(d_starts);
    out.ctx = ctx;
    out.target_name = hdr.name;
    out.target_len = hdr.len;
    out.n_ref = static_cast<int32_t>(hdr.name.size());
    out.n_records = kept;
    out.stop = out.total = total;
    out.first = static_cast<int64_t>(head.size());
    out.d_stream = d_stream;
    out.d_starts = d_starts;
    if (n_dropped_out) *n_dropped_out = res[1];
}

}  // namespace palace_host
