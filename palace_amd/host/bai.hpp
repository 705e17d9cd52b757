// The .bai of a coordinate-sorted BAM whose inflated stream and record starts lie in device memory (`bamsort --bai`, `bamsort --index`;
// the driver's `samtools index`, palace:433).  Written from the SAM specification, section 5.2; the rules are DESIGN.md 8.  Everything
// that depends on the records is computed where they lie:
//     palace_bai_records     what each record is filed under; records a .bai cannot hold; the order check
//     palace_bai_chunks      runs of equal (refID, bin) as chunks, ordered by (refID, bin, file order): counted, then written
//     palace_bai_linear      per reference: windows, mapped / unmapped counts, first and last offset; then the 16 kb linear index
//     palace_bgzf_voffsets   stream offsets -> virtual offsets, from the file's member table
// The host copies the arrays back and lays them out as the file's bytes.  Every bin keeps its own chunks: htslib also folds sparsely
// filled bins into their parents, so the bytes are not its bytes; any reader of the format looks through every level.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_scope.hpp"

namespace palace_host {

// the out-of-room text of bamsort's steps (and of the member writer behind samview)
inline std::string bamsort_no_room(size_t bytes, const char *what, const char *err)
{
    return "the inflated BAM, the sorted stream, the per-record arrays and one batch of members are kept on the device, and " + std::to_string(bytes) +
           " bytes for " + what + " cannot be allocated (" + err + "); there is no host path, a BAM larger than device memory is out of scope";
}

constexpr uint32_t kBaiPseudoBin = 37450;

// file: the BAM's name for messages.  member_u / member_c: stream offset and file offset of every BGZF member, the last entry standing
// for the stream's end (palace_bgzf_voffsets).  Throws std::runtime_error; nothing is written unless everything was computed.
inline void write_bai_device(palace_ctx *ctx, const std::string &file, const uint8_t *d_stream, const int64_t *d_starts, int64_t n_records, int32_t n_ref,
                             const std::vector<int64_t> &member_u, const std::vector<int64_t> &member_c, const std::string &bai_path)
{
    DeviceScope dev(ctx, bamsort_no_room);
    const size_t n = static_cast<size_t>(n_records), nr = static_cast<size_t>(n_ref);
    int32_t *d_ref = dev.array<int32_t>(n, "the index columns"), *d_bin = dev.array<int32_t>(n, "the index columns");
    int32_t *d_wb = dev.array<int32_t>(n, "the index columns"), *d_we = dev.array<int32_t>(n, "the index columns");
    uint8_t *d_unm = dev.array<uint8_t>(n, "the index columns");
    palace_bai_status st;
    ck(palace_bai_records(ctx, d_stream, d_starts, n_records, n_ref, d_ref, d_bin, d_wb, d_we, d_unm, &st), "palace_bai_records");
    if (st.n_bad) throw std::runtime_error("record " + std::to_string(st.first_bad) + ": outside what a .bai can index (" + std::to_string(st.n_bad) + " such records)");
    if (st.first_unsorted >= 0) throw std::runtime_error(file + " is not coordinate-sorted (record " + std::to_string(st.first_unsorted) + ")");

    // chunks: counted, then written
    int64_t n_runs = 0, again = 0;
    ck(palace_bai_chunks(ctx, d_stream, d_starts, d_ref, d_bin, n_records, n_ref, nullptr, nullptr, nullptr, nullptr, 0, &n_runs), "palace_bai_chunks");
    const size_t nc = static_cast<size_t>(n_runs);
    int32_t *d_cref = dev.array<int32_t>(nc, "the chunks"), *d_cbin = dev.array<int32_t>(nc, "the chunks");
    int64_t *d_cbeg = dev.array<int64_t>(nc, "the chunks"), *d_cend = dev.array<int64_t>(nc, "the chunks");
    if (n_runs) {
        ck(palace_bai_chunks(ctx, d_stream, d_starts, d_ref, d_bin, n_records, n_ref, d_cref, d_cbin, d_cbeg, d_cend, n_runs, &again), "palace_bai_chunks");
        if (again != n_runs) throw std::runtime_error("palace_bai_chunks: two counts of one stream differ");
    }

    // per reference: windows and the pseudo-bin's numbers; then the linear index
    int32_t *d_n_intv = dev.array<int32_t>(nr, "the references' windows");
    int64_t *d_stat = dev.array<int64_t>(4 * nr, "the references' numbers");
    ck(palace_bai_linear(ctx, d_stream, d_starts, d_ref, d_wb, d_we, d_unm, n_records, n_ref, d_n_intv, d_stat, nullptr, 0, nullptr), "palace_bai_linear");
    std::vector<int32_t> n_intv(nr);
    if (nr) ck(palace_d2h(ctx, n_intv.data(), d_n_intv, nr * 4), "palace_d2h");
    std::vector<int64_t> lin_off(nr + 1, 0);
    for (size_t t = 0; t < nr; t++) lin_off[t + 1] = lin_off[t] + n_intv[t];
    const size_t nl = static_cast<size_t>(lin_off[nr]);
    const int64_t *d_lin_off = dev.upload(lin_off.data(), nr + 1, "the linear index");
    int64_t *d_lin = dev.array<int64_t>(nl, "the linear index");
    ck(palace_bai_linear(ctx, d_stream, d_starts, d_ref, d_wb, d_we, d_unm, n_records, n_ref, d_n_intv, d_stat, d_lin_off, static_cast<int64_t>(nl), d_lin),
       "palace_bai_linear");

    // virtual offsets
    const size_t nm = member_u.size();
    const int64_t *d_mu = dev.upload(member_u.data(), nm, "the member table"), *d_mc = dev.upload(member_c.data(), nm, "the member table");
    auto voffsets = [&](const int64_t *d_u, size_t count) {
        std::vector<uint64_t> v(count);
        if (!count) return v;
        uint64_t *d_v = dev.array<uint64_t>(count, "the virtual offsets");
        ck(palace_bgzf_voffsets(ctx, d_u, static_cast<int64_t>(count), d_mu, d_mc, static_cast<int64_t>(nm), d_v), "palace_bgzf_voffsets");
        ck(palace_d2h(ctx, v.data(), d_v, count * 8), "palace_d2h");
        dev.give_back(d_v);
        return v;
    };
    const std::vector<uint64_t> cbeg = voffsets(d_cbeg, nc), cend = voffsets(d_cend, nc), lin = voffsets(d_lin, nl);
    const std::vector<uint64_t> first = voffsets(d_stat + 2 * nr, nr), last = voffsets(d_stat + 3 * nr, nr);
    std::vector<int32_t> cref(nc), cbin(nc);
    std::vector<int64_t> counts(2 * nr);
    if (nc) { ck(palace_d2h(ctx, cref.data(), d_cref, nc * 4), "palace_d2h"); ck(palace_d2h(ctx, cbin.data(), d_cbin, nc * 4), "palace_d2h"); }
    if (nr) ck(palace_d2h(ctx, counts.data(), d_stat, 2 * nr * 8), "palace_d2h");

    // the file's bytes
    std::vector<uint8_t> b;
    auto put = [&b](uint64_t v, int bytes) { for (int k = 0; k < bytes; k++) b.push_back(static_cast<uint8_t>(v >> (8 * k))); };
    b.insert(b.end(), {'B', 'A', 'I', 1});
    put(static_cast<uint32_t>(n_ref), 4);
    size_t c = 0;
    for (size_t t = 0; t < nr; t++) {
        size_t e = c, bins = 0;
        while (e < nc && cref[e] == static_cast<int32_t>(t)) { if (e == c || cbin[e] != cbin[e - 1]) bins++; e++; }
        if (e == c) { put(0, 4); put(0, 4); continue; }                      // a reference without records
        put(bins + 1, 4);
        while (c < e) {
            size_t g = c;
            while (g < e && cbin[g] == cbin[c]) g++;
            put(static_cast<uint32_t>(cbin[c]), 4);
            put(g - c, 4);
            for (; c < g; c++) { put(cbeg[c], 8); put(cend[c], 8); }
        }
        put(kBaiPseudoBin, 4); put(2, 4);
        put(first[t], 8); put(last[t], 8);
        put(static_cast<uint64_t>(counts[t]), 8); put(static_cast<uint64_t>(counts[nr + t]), 8);
        put(static_cast<uint32_t>(n_intv[t]), 4);
        for (int64_t w = lin_off[t]; w < lin_off[t + 1]; w++) put(lin[static_cast<size_t>(w)], 8);
    }
    put(static_cast<uint64_t>(st.n_no_coor), 8);
    FILE *f = std::fopen(bai_path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot open " + bai_path + " for writing");
    const bool ok = std::fwrite(b.data(), 1, b.size(), f) == b.size();
    if (std::fclose(f) != 0 || !ok) { std::remove(bai_path.c_str()); throw std::runtime_error("write failed: " + bai_path); }
}

}  // namespace palace_host
