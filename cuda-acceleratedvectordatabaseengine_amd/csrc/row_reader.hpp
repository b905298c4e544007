// row_reader.hpp — the screened tier's survivor-row reads from the index file: host logic
// only (no HIP), so the CPU tests drive it on a file of their own (tests/cpp/row_reader_test.cpp).
//
// One operation: read a list of fp32 rows, each `row_bytes` long at its own file offset, to
// their rows of a staging buffer, with at most `qd` reads queued or in flight on a ring of
// the reader's own. Buffered (no O_DIRECT descriptor): each read lands in its staging row.
// O_DIRECT: each read is the row's aligned superset (the file system's granule) into one
// bounce slot per read in flight, and the row is copied out on completion. A read succeeds
// when it delivered the row's last byte, so a superset cut short by the end of the file is
// fine. On any failure every read still queued or in flight is waited for and dropped
// before the error leaves, so the reader serves the next call.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "uring.hpp"

namespace vdbe {

// the aligned superset [a0, a1) of [off, off + len) for an O_DIRECT granule g
inline void aligned_superset(uint64_t off, uint64_t len, uint64_t g, uint64_t& a0, uint64_t& a1) {
    a0 = off / g * g;
    a1 = (off + len + g - 1) / g * g;
}

class RowReader {
public:
    struct Req {
        uint64_t off;  // the row's offset in the file
        uint32_t row;  // its row in the staging
    };
    // a read that did not deliver its row (the engine reports it as a state error)
    struct ShortRead : std::runtime_error {
        using std::runtime_error::runtime_error;
    };

    // one bounce slot: the row's 4 KiB pages plus one (a row may start anywhere in its first)
    static uint64_t slot_bytes(uint64_t row_bytes) { return ((row_bytes + 4095) / 4096 + 1) * 4096; }

    // Reads in flight for a requested depth (the ring is created, or recreated when it is
    // smaller than asked for), and the bounce bytes read_rows needs for them with O_DIRECT
    // (the slots plus the slack to round the base up to 4 KiB).
    uint32_t depth(uint32_t qd) {
        if (ring_ && ring_->capacity() < qd) ring_.reset();
        if (!ring_) ring_.reset(new UringReader(qd));
        return std::min(qd, ring_->capacity());
    }
    uint64_t bounce_bytes(uint32_t qd, uint64_t row_bytes) { return depth(qd) * slot_bytes(row_bytes) + 4096; }

    // Read every request's row to stage + row * row_bytes, in the order given. fd_direct >= 0:
    // O_DIRECT reads of granule g through `bounce` (bounce_bytes() long); else buffered reads
    // on fd. Returns the bytes the device delivered: the aligned supersets, or the rows.
    uint64_t read_rows(int fd, int fd_direct, uint32_t g, uint32_t qd, uint64_t row_bytes,
                       const std::vector<Req>& reqs, char* stage, char* bounce) {
        const bool direct = fd_direct >= 0;
        const uint32_t kQD = depth(qd);
        UringReader* const ur = ring_.get();
        const uint64_t span = slot_bytes(row_bytes);
        bounce = (char*)(((uintptr_t)bounce + 4095) & ~(uintptr_t)4095);
        free_slots_.resize(kQD);
        for (uint32_t b = 0; b < kQD; ++b) free_slots_[b] = kQD - 1 - b;
        delta_.resize(kQD);
        uint64_t bytes_read = 0;
        const size_t n = reqs.size();
        size_t next = 0, done = 0;
        try {
            while (done < n) {
                while (next < n && next - done < kQD) {  // (<= kQD queued or in flight)
                    const Req& r = reqs[next];
                    if (direct) {
                        const uint32_t b = free_slots_.back();
                        free_slots_.pop_back();
                        uint64_t a0, a1;
                        aligned_superset(r.off, row_bytes, g, a0, a1);
                        delta_[b] = r.off - a0;
                        ur->read(fd_direct, bounce + (size_t)b * span, (uint32_t)(a1 - a0), a0, ((uint64_t)b << 32) | r.row);
                        bytes_read += a1 - a0;
                    } else {
                        ur->read(fd, stage + (size_t)r.row * row_bytes, (uint32_t)row_bytes, r.off, r.row);
                        bytes_read += row_bytes;
                    }
                    ++next;
                }
                for (const UringReader::Done& d : ur->wait(1)) {
                    const uint32_t b = (uint32_t)(d.tag >> 32), row = (uint32_t)d.tag;
                    const int64_t want = direct ? (int64_t)(delta_[b] + row_bytes) : (int64_t)row_bytes;
                    if (d.result < want)
                        throw ShortRead("short read of a survivor row from the list file" +
                                        (d.result < 0 ? std::string(": ") + std::strerror((int)-d.result) : ""));
                    if (direct) {
                        std::memcpy(stage + (size_t)row * row_bytes, bounce + (size_t)b * span + delta_[b], row_bytes);
                        free_slots_.push_back(b);
                    }
                    ++done;
                }
            }
        } catch (...) {
            ur->drain();
            throw;
        }
        return bytes_read;
    }

private:
    std::unique_ptr<UringReader> ring_;
    std::vector<uint32_t> free_slots_;  // bounce slots no read in flight uses
    std::vector<uint64_t> delta_;       // per bounce slot: where its row starts in it
};

}  // namespace vdbe
