// A file mapped read-only (no copy of it is made).  The access hint and the two message prefixes are the caller's: text inputs are
// populated and say `cannot open <path>` / `cannot read <path>`, a BAM is read front to back and says `Failed to open BAM <path>` /
// `Failed to read BAM <path>`.  An empty file is size 0 with no mapping.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace palace_host {

enum class MapHint { none, populate, sequential };

struct MappedFile {
    const char *data = nullptr;
    size_t size = 0;
    MappedFile() = default;
    explicit MappedFile(const std::string &path, MapHint hint = MapHint::populate, const char *open_msg = "cannot open ", const char *read_msg = "cannot read ")
    {
        open(path, hint, open_msg, read_msg);
    }
    void open(const std::string &path, MapHint hint = MapHint::populate, const char *open_msg = "cannot open ", const char *read_msg = "cannot read ")
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error(open_msg + path);
        struct stat st;
        if (::fstat(fd, &st) != 0) { ::close(fd); throw std::runtime_error(open_msg + path); }
        size = static_cast<size_t>(st.st_size);
        if (size) {
            void *m = ::mmap(nullptr, size, PROT_READ, MAP_PRIVATE | (hint == MapHint::populate ? MAP_POPULATE : 0), fd, 0);
            if (m == MAP_FAILED) { ::close(fd); throw std::runtime_error(read_msg + path); }
            if (hint == MapHint::sequential) ::madvise(m, size, MADV_SEQUENTIAL);
            data = static_cast<const char *>(m);
        }
        ::close(fd);
    }
    const uint8_t *bytes() const { return reinterpret_cast<const uint8_t *>(data); }
    ~MappedFile() { if (data) ::munmap(const_cast<char *>(data), size); }
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};
using MappedText = MappedFile;                       // the text inputs' name for it (the defaults are theirs)

}  // namespace palace_host
