// The grammar of one line of `samtools depth` text, stated once: `name <TAB> position <TAB> depth`, the LF not part of it.  This one
// text is compiled by hipcc for the kernels of depth_parse.hip and by the host compiler for `hostdump depthline` (and its sanitizer
// build), so the device, the CPU tests and the sanitizer run check the same rules.
//   name      1 or more bytes, none of them TAB (an LF cannot be inside a line);
//   position  1-10 decimal digits, value <= 2^31 - 1 (not otherwise looked at);
//   depth     1-10 decimal digits, value <= 2^31 - 1 (0 is a depth: `samtools depth -a` writes it);
//   the line  at most kDepthLineMax bytes, its LF counted: what a parser carries from one window of the file to the next.
// Anything else is a bad line: no sign, no space, no CR, no third number, no missing column.
// The line is read from its END, as the kernel's lanes find it (a lane owns the LF and walks back): depth, position, name.  No
// allocation, no library call, nothing of HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PALACE_DEPTH_FN __device__ __forceinline__
#else
#define PALACE_DEPTH_FN inline
#endif

namespace palace {

constexpr int kDepthLineMax = 4096;                  // bytes of a line, LF included
constexpr uint32_t kDepthValueMax = 0x7fffffffu;

enum DepthLineError : int32_t {
    kDepthLineOk = 0,
    kDepthLineEmpty,        // no byte at all
    kDepthLineColumns,      // fewer or more than three columns, or an empty name
    kDepthLineNumber,       // an empty number, or a byte in it that is no digit
    kDepthLineDigits,       // more than 10 digits
    kDepthLineValue,        // a value of 2^31 or more
    kDepthLineLong          // longer than kDepthLineMax
};

struct DepthLine {
    int64_t start;          // index of the line's first byte
    int32_t name_len;       // the name is get(start .. start + name_len)
    uint32_t pos, depth;
    int32_t error;          // DepthLineError; the three fields above hold nothing when it is not kDepthLineOk
};

// The line that ends in front of index `end` (where its LF is, or the text ends), of a text whose byte i is get(i) for i >= lo:
// walks back from end - 1 to the byte behind the previous LF, or to lo.  `start` is right for every line that is not too long.
template <class Get>
PALACE_DEPTH_FN DepthLine depth_line_back(Get get, int64_t lo, int64_t end)
{
    DepthLine r{end, 0, 0u, 0u, kDepthLineOk};
    int field = 2;                                   // 2: depth, 1: position, 0: name
    int digits = 0;
    uint64_t value = 0, unit = 1;
    int32_t err = kDepthLineOk;
    int64_t i = end, name_end = end;
    while (i > lo) {
        const uint32_t c = get(i - 1);
        if (c == '\n') break;
        i--;
        if (end - i > kDepthLineMax - 1) { err = kDepthLineLong; break; }
        if (err) continue;                           // (the start is still looked for)
        if (field == 0) {
            if (c == '\t') err = kDepthLineColumns;  // a fourth column
            continue;
        }
        if (c == '\t') {
            if (digits == 0) err = kDepthLineNumber;
            else if (value > kDepthValueMax) err = kDepthLineValue;
            if (field == 2) r.depth = static_cast<uint32_t>(value); else { r.pos = static_cast<uint32_t>(value); name_end = i; }
            field--; digits = 0; value = 0; unit = 1;
            continue;
        }
        if (c < '0' || c > '9') { err = kDepthLineNumber; continue; }
        if (++digits > 10) { err = kDepthLineDigits; continue; }
        value += (c - '0') * unit;
        unit *= 10;
    }
    r.start = i;
    if (err == kDepthLineOk) {
        if (end == i) err = kDepthLineEmpty;
        else if (field != 0) err = kDepthLineColumns;                      // one or two columns
        else if (name_end == i) err = kDepthLineColumns;                   // an empty name
    }
    r.name_len = err ? 0 : static_cast<int32_t>(name_end - i);
    r.error = err;
    return r;
}

// a line held in memory: p[0 .. len), no LF inside
PALACE_DEPTH_FN DepthLine depth_line_parse(const uint8_t *p, int64_t len)
{
    return depth_line_back([p](int64_t i) { return static_cast<uint32_t>(p[i]); }, 0, len);
}

PALACE_DEPTH_FN const char *depth_line_error_text(int32_t e)
{
    switch (e) {
    case kDepthLineOk: return "ok";
    case kDepthLineEmpty: return "empty line";
    case kDepthLineColumns: return "not three columns with a name in the first";
    case kDepthLineNumber: return "a position or depth that is not 1-10 decimal digits";
    case kDepthLineDigits: return "a number of more than 10 digits";
    case kDepthLineValue: return "a number above 2147483647";
    default: return "a line longer than 4096 bytes";
    }
}

}  // namespace palace
