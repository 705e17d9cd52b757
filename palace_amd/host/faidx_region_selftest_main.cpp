// csrc/faidx_region.hpp on a CPU (tests/test_host_faidx_rules.py), as built and under the host sanitizers; nothing of the device is
// linked.
//   faidx_region_selftest <records> <regions>    records: one `name TAB length` per line, in file order (of equal names the first
//                                                is found); regions: one region per line (cut at LF, a last line without LF is a
//                                                line), each copied into an allocation of exactly its length: `rec beg len`
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../csrc/faidx_region.hpp"

namespace {

bool read_all(const char *path, std::string &text)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return false; }
    char buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    std::fclose(f);
    return true;
}

// f(line) for every line of the text
template <class F> void for_lines(const std::string &text, F f)
{
    for (size_t a = 0; a < text.size();) {
        const size_t lf = text.find('\n', a), e = lf == std::string::npos ? text.size() : lf;
        f(text.substr(a, e - a));
        a = e + 1;
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fputs("usage: faidx_region_selftest <records: name TAB length per line> <regions: one per line>\n", stderr);
        return 2;
    }
    std::string records, regions;
    if (!read_all(argv[1], records) || !read_all(argv[2], regions)) return 1;
    std::map<std::string, int64_t> first_of;
    std::vector<int64_t> length;
    for_lines(records, [&](const std::string &line) {
        const size_t tab = line.rfind('\t');
        first_of.emplace(line.substr(0, tab), static_cast<int64_t>(length.size()));
        length.push_back(std::strtoll(line.c_str() + tab + 1, nullptr, 10));
    });
    for_lines(regions, [&](const std::string &line) {
        const std::vector<uint8_t> region(line.begin(), line.end());         // (exactly the region: a read past it is the sanitizer's)
        const palace::FaidxRegion g = palace::faidx_region_resolve(
            region.data(), static_cast<int64_t>(region.size()),
            [&](const uint8_t *p, int64_t n) -> int64_t {
                if (n <= 0) return -1;
                const auto it = first_of.find(std::string(reinterpret_cast<const char *>(p), static_cast<size_t>(n)));
                return it == first_of.end() ? -1 : it->second;
            },
            [&](int64_t r) { return length[static_cast<size_t>(r)]; });
        std::printf("%lld %lld %lld\n", static_cast<long long>(g.rec), static_cast<long long>(g.beg), static_cast<long long>(g.len));
    });
    return 0;
}
