// CPU unit test of the screened tier's survivor-row reads (csrc/row_reader.hpp) on a file
// of its own under the directory given as argv[1]: an unaligned header, then rows whose
// bytes are a function of the row index. Buffered and O_DIRECT (granules 4096 and, where
// the file system takes it, 512), rows of 280 and 3072 bytes, 1, 3 and 256 reads in flight,
// a shuffled subset read to other rows of the staging, the file's last row (its aligned
// superset runs past the end), an empty list, the delivered byte count, a file cut through
// a requested row, a bad descriptor, and the same reader serving a valid list after each
// failure. Exit status 0 = every check passed. Built and run by tests/test_row_reader.py
// with g++ (no GPU), once plain and once with the address and undefined-behaviour sanitizers.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/row_reader.hpp"

using vdbe::RowReader;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static const uint32_t kRows = 1000;
static const uint64_t kHeader = 24 + 8 * (uint64_t)kRows;  // (the index file's: not a multiple of 512)
static const uint8_t kSentinel = 0xA5;

static uint8_t row_byte(uint32_t row, uint64_t j) { return (uint8_t)(row * 131u + (row >> 8) * 17u + j * 7u + 3u); }

static std::string write_file(const std::string& dir, uint64_t row_bytes, uint64_t cut_at = 0) {
    const std::string path = dir + "/rows_" + std::to_string(row_bytes) + (cut_at ? "_cut" : "") + ".bin";
    std::vector<uint8_t> buf(kHeader + kRows * row_bytes);
    for (uint64_t i = 0; i < kHeader; ++i) buf[i] = (uint8_t)(i * 29u + 1u);
    for (uint32_t r = 0; r < kRows; ++r)
        for (uint64_t j = 0; j < row_bytes; ++j) buf[kHeader + r * row_bytes + j] = row_byte(r, j);
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(buf.data(), 1, cut_at ? cut_at : buf.size(), f) != (cut_at ? cut_at : buf.size())) {
        std::printf("cannot write %s\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return path;
}

struct Aligned {  // page-aligned host memory (the engine's is page-locked)
    char* p = nullptr;
    explicit Aligned(size_t bytes) {
        void* v = nullptr;
        if (posix_memalign(&v, 4096, std::max<size_t>(bytes, 1)) != 0) std::exit(2);
        p = (char*)v;
    }
    ~Aligned() { std::free(p); }
};

struct Leg {
    int fd, fd_direct;
    uint32_t g;
    uint64_t row_bytes;
};

// `n` distinct rows of the file (the last one among them) in shuffled order, each to its
// own row of a staging of n + 40 rows, not the identity
static std::vector<RowReader::Req> requests(uint32_t n, uint64_t row_bytes, uint32_t seed, uint32_t& stage_rows) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> src(kRows - 1), dst(n + 40);
    std::iota(src.begin(), src.end(), 0u);
    std::iota(dst.begin(), dst.end(), 0u);
    std::shuffle(src.begin(), src.end(), rng);
    std::shuffle(dst.begin(), dst.end(), rng);
    src[n / 2] = kRows - 1;
    std::vector<RowReader::Req> reqs(n);
    for (uint32_t i = 0; i < n; ++i) reqs[i] = {kHeader + src[i] * row_bytes, dst[i]};
    stage_rows = n + 40;
    return reqs;
}

// the bytes the device delivers for these requests, by block numbers
static uint64_t expected_bytes(const Leg& leg, const std::vector<RowReader::Req>& reqs) {
    if (leg.fd_direct < 0) return reqs.size() * leg.row_bytes;
    uint64_t sum = 0;
    for (const auto& r : reqs) sum += ((r.off + leg.row_bytes - 1) / leg.g - r.off / leg.g + 1) * leg.g;
    return sum;
}

// read the requests and check every staging byte: the row where one was asked for, the
// sentinel elsewhere
static void read_and_check(RowReader& rd, const Leg& leg, uint32_t qd, const std::vector<RowReader::Req>& reqs,
                           uint32_t stage_rows) {
    const uint64_t rb = leg.row_bytes;
    Aligned stage(stage_rows * rb);
    std::memset(stage.p, kSentinel, stage_rows * rb);
    // (a bounce base that is not 4 KiB-aligned: the reader rounds it up within its slack)
    Aligned bounce(rd.bounce_bytes(qd, rb) + 64);
    const uint64_t got = rd.read_rows(leg.fd, leg.fd_direct, leg.g, qd, rb, reqs, stage.p, bounce.p + 64);
    CHECK(got == expected_bytes(leg, reqs));
    std::vector<int64_t> src_of(stage_rows, -1);
    for (const auto& r : reqs) src_of[r.row] = (int64_t)((r.off - kHeader) / rb);
    uint64_t bad = 0;
    for (uint32_t d = 0; d < stage_rows; ++d)
        for (uint64_t j = 0; j < rb; ++j) {
            const uint8_t want = src_of[d] < 0 ? kSentinel : row_byte((uint32_t)src_of[d], j);
            bad += (uint8_t)stage.p[d * rb + j] != want;
        }
    CHECK(bad == 0);
}

static void good_legs(RowReader& rd, const Leg& leg) {
    for (uint32_t qd : {1u, 3u, 256u})
        for (uint32_t n : {300u, 100u}) {  // (more and fewer requests than 256 in flight)
            uint32_t stage_rows = 0;
            const auto reqs = requests(n, leg.row_bytes, 7 * qd + n, stage_rows);
            read_and_check(rd, leg, qd, reqs, stage_rows);
        }
    // the last row alone, and no request at all
    read_and_check(rd, leg, 3, {{kHeader + (uint64_t)(kRows - 1) * leg.row_bytes, 2}}, 4);
    Aligned stage(4 * leg.row_bytes), bounce(rd.bounce_bytes(3, leg.row_bytes));
    std::memset(stage.p, kSentinel, 4 * leg.row_bytes);
    CHECK(rd.read_rows(leg.fd, leg.fd_direct, leg.g, 3, leg.row_bytes, {}, stage.p, bounce.p) == 0);
    uint64_t touched = 0;
    for (uint64_t j = 0; j < 4 * leg.row_bytes; ++j) touched += (uint8_t)stage.p[j] != kSentinel;
    CHECK(touched == 0);
}

// a failing call: it throws a message holding `what`; then the reader serves a valid list
static void failing_leg(RowReader& rd, const Leg& bad, const std::vector<RowReader::Req>& reqs, uint32_t stage_rows,
                        const std::string& what, const Leg& good) {
    for (uint32_t qd : {1u, 3u, 256u}) {
        Aligned stage(stage_rows * bad.row_bytes), bounce(rd.bounce_bytes(qd, bad.row_bytes));
        bool threw = false;
        try {
            (void)rd.read_rows(bad.fd, bad.fd_direct, bad.g, qd, bad.row_bytes, reqs, stage.p, bounce.p);
        } catch (const std::runtime_error& e) {
            threw = true;
            if (std::string(e.what()).find(what) == std::string::npos) {
                std::printf("FAIL: message \"%s\" lacks \"%s\"\n", e.what(), what.c_str());
                ++failures;
            }
        }
        CHECK(threw);
        uint32_t rows = 0;
        const auto ok = requests(100, good.row_bytes, 1000 + qd, rows);
        read_and_check(rd, good, qd, ok, rows);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s <directory>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    RowReader rd;  // (one reader throughout: its ring grows with the depth asked for)
    for (uint64_t rb : {(uint64_t)280, (uint64_t)3072}) {
        const std::string path = write_file(dir, rb);
        const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd < 0) {
            std::printf("cannot open %s\n", path.c_str());
            return 2;
        }
        const int fdd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC | O_DIRECT);
        const int fdd_errno = errno;
        bool g512 = false;
        if (fdd >= 0) {  // (as the engine probes: a 512-B read at a 512-B offset, accepted or EINVAL)
            Aligned pb(4096);
            g512 = ::pread(fdd, pb.p, 512, 512) == 512;
        }
        std::vector<Leg> legs = {{fd, -1, 4096, rb}};
        if (fdd >= 0) legs.push_back({fd, fdd, 4096, rb});
        if (g512) legs.push_back({fd, fdd, 512, rb});
        for (const Leg& leg : legs) good_legs(rd, leg);

        // a file cut through the middle of row 500: rows before it read, row 500 does not
        const uint32_t cut_row = 500;
        const std::string cut = write_file(dir, rb, kHeader + cut_row * rb + rb / 2);
        const int cfd = ::open(cut.c_str(), O_RDONLY | O_CLOEXEC);
        const int cfdd = fdd >= 0 ? ::open(cut.c_str(), O_RDONLY | O_CLOEXEC | O_DIRECT) : -1;
        CHECK(cfd >= 0 && (fdd < 0 || cfdd >= 0));
        std::vector<RowReader::Req> reqs;
        for (uint32_t i = 0; i < 20; ++i) reqs.push_back({kHeader + (uint64_t)(cut_row - 12 + i) * rb, 19 - i});
        // a descriptor that is not open
        int closed = ::open("/dev/null", O_RDONLY | O_CLOEXEC);
        ::close(closed);
        for (const Leg& leg : legs) {
            const Leg cut_leg = {cfd, leg.fd_direct < 0 ? -1 : cfdd, leg.g, rb};
            failing_leg(rd, cut_leg, reqs, 20, "short read of a survivor row", leg);
            const Leg bad_leg = {closed, leg.fd_direct < 0 ? -1 : closed, leg.g, rb};
            failing_leg(rd, bad_leg, reqs, 20, std::string(": ") + std::strerror(EBADF), leg);
        }
        std::printf("row_bytes %llu: buffered: ok\n", (unsigned long long)rb);
        if (fdd < 0)
            std::printf("row_bytes %llu: O_DIRECT open failed (%s): buffered legs only\n", (unsigned long long)rb,
                        std::strerror(fdd_errno));
        else
            std::printf("row_bytes %llu: direct 4096: ok, direct 512: %s\n", (unsigned long long)rb,
                        g512 ? "ok" : "refused by the file system");
        ::close(fd);
        ::close(cfd);
        if (fdd >= 0) ::close(fdd);
        if (cfdd >= 0) ::close(cfdd);
    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
