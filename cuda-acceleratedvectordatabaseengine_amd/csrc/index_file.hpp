// index_file.hpp — the on-disk index format, written and read in one place: host logic only
// (no HIP), so the CPU tests pin every byte and offset and feed the reader cut and hostile
// files (tests/cpp/index_file_test.cpp). The format is this engine's own (the reference
// declares load() and never defines it); this comment is its normative description.
//
// All integers are little-endian, floats are IEEE fp32, nothing is padded or aligned.
//
//   Index file (vdb_ivf_save of a group or an unsharded handle):
//     char magic[8] = "VDBIVF01"; u32 dim; u32 nlist; i32 metric; u32 reserved (0)   24 bytes
//     f32 centroids[nlist][dim]
//     per list 0 .. nlist-1:  u64 count; u64 ids[count]; f32 vectors[count][dim]
//
//   Shard file (vdb_ivf_save of a sharded handle, world > 1: one rank's lists):
//     char magic[8] = "VDBIVS01"; u32 dim; u32 nlist; i32 metric; u32 rank; u32 world;
//     u32 reserved (0)                                                               32 bytes
//     f32 centroids[nlist][dim]
//     per list:  u64 count (global: emptiness semantics); u64 stored (count if the rank owns
//                the list, else 0); u64 ids[stored]; f32 vectors[stored][dim]
//
// metric is the configured one (vdb_ivf_config::metric; 3 = CosineDistance, whose rows are
// stored as unit rows). Rows stand in add order. Bytes after the last list are ignored.
//
// The engine keeps the descriptors, the O_DIRECT probing, the staging rings and everything
// that touches the device; it hands the reader a "read n bytes at offset o" callable and the
// writer a "put bytes" callable, and maps the refusals below to its error codes.
#pragma once
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <vector>

namespace vdbe {

// A file shorter than its headers claim (64-bit overflow of a claim included).
struct IndexFileTruncated : std::runtime_error {
    IndexFileTruncated() : std::runtime_error("truncated index file") {}
};
// A file that is whole but not one this handle can take; one type per reason.
struct IndexFileRefused : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct IndexFileBadMagic : IndexFileRefused {  // (reported like any other file that does not fit)
    IndexFileBadMagic() : IndexFileRefused("index file does not match this index's configuration") {}
};
struct IndexFileMismatch : IndexFileRefused {
    IndexFileMismatch() : IndexFileRefused("index file does not match this index's configuration") {}
};
struct IndexFileBadShard : IndexFileRefused {
    IndexFileBadShard() : IndexFileRefused("shard file with an invalid (rank, world)") {}
};
struct IndexFilePartialList : IndexFileRefused {
    IndexFilePartialList() : IndexFileRefused("shard file stores part of a list") {}
};

struct IndexFileHeader {
    static constexpr const char* kIndexMagic = "VDBIVF01";
    static constexpr const char* kShardMagic = "VDBIVS01";
    static constexpr uint64_t kMagicBytes = 8, kIndexBytes = 24, kShardBytes = 32;
    static constexpr uint64_t kIdBytes = 8;  // one id, and one count

    bool shard = false;
    uint32_t dim = 0, nlist = 0;
    int32_t metric = 0;
    uint32_t rank = 0, world = 1;  // (a shard file's; an index file is rank 0 of 1)

    uint64_t bytes() const { return shard ? kShardBytes : kIndexBytes; }
    uint64_t list_header_bytes() const { return shard ? 2 * kIdBytes : kIdBytes; }  // count[, stored]
    uint64_t row_bytes() const { return (uint64_t)dim * 4; }

    // The header's bytes() bytes into `out` (kShardBytes long at least).
    void encode(unsigned char* out) const {
        const uint32_t w[6] = {dim, nlist, (uint32_t)metric, shard ? rank : 0, shard ? world : 0, 0};
        std::memcpy(out, shard ? kShardMagic : kIndexMagic, kMagicBytes);
        std::memcpy(out + kMagicBytes, w, bytes() - kMagicBytes);
    }
    // Which variant the first kMagicBytes bytes announce.
    static bool shard_magic(const unsigned char* magic) {
        if (std::memcmp(magic, kShardMagic, kMagicBytes) == 0) return true;
        if (std::memcmp(magic, kIndexMagic, kMagicBytes) != 0) throw IndexFileBadMagic();
        return false;
    }
    // From a whole header (bytes() of the variant its magic announces).
    static IndexFileHeader decode(const unsigned char* in) {
        IndexFileHeader h;
        h.shard = shard_magic(in);
        uint32_t w[6] = {0, 0, 0, 0, 0, 0};
        std::memcpy(w, in + kMagicBytes, h.bytes() - kMagicBytes);
        h.dim = w[0];
        h.nlist = w[1];
        h.metric = (int32_t)w[2];
        if (h.shard) h.rank = w[3], h.world = w[4];
        return h;
    }
    // The one configuration match: a handle takes only a file of its dimension, list count
    // and configured metric.
    void require_config(uint32_t want_dim, uint32_t want_nlist, int want_metric) const {
        if (dim != want_dim || nlist != want_nlist || metric != want_metric) throw IndexFileMismatch();
    }
};

// Where everything lies in one file, from its header and its per-list headers.
struct IndexFileDirectory {
    struct List {
        uint64_t count;    // the list's rows in the whole index
        uint64_t stored;   // its rows in this file: count, or 0 (a shard file, another rank's list)
        uint64_t ids_off;  // file offset of its ids (its vectors follow them)
    };
    IndexFileHeader header;
    std::vector<List> lists;
    uint64_t centroids_off = 0;
    uint64_t end = 0;  // one past the last list's last row: no file of this content is shorter

    uint64_t centroid_bytes() const { return (uint64_t)header.nlist * header.row_bytes(); }
    uint64_t ids_offset(uint32_t l, uint64_t r) const { return lists[l].ids_off + r * IndexFileHeader::kIdBytes; }
    uint64_t row_offset(uint32_t l, uint64_t r) const {
        return lists[l].ids_off + lists[l].stored * IndexFileHeader::kIdBytes + r * header.row_bytes();
    }
    // A shard file's rank owns the lists whose rows it stores (any plan); an index file's, all.
    bool owned(uint32_t l) const { return !header.shard || (lists[l].count != 0 && lists[l].stored == lists[l].count); }
};

// at + n * each for the reader's walk: IndexFileTruncated once that passes `size` or 64 bits.
inline uint64_t index_file_advance(uint64_t at, uint64_t n, uint64_t each, uint64_t size) {
    uint64_t b = 0, to = 0;
    if (__builtin_mul_overflow(n, each, &b) || __builtin_add_overflow(at, b, &to) || to > size) throw IndexFileTruncated();
    return to;
}

// The reader, in two steps so that a caller can judge the header before the lists are walked.
// read(off, dst, n) delivers n bytes at offset off or throws; `size` is the file's. Nothing at
// or past `size` is asked for, and nothing is allocated for a count before the file's size
// has vouched for it. Refusals: IndexFileBadMagic, IndexFileTruncated; then IndexFileBadShard
// (world == 0 or rank >= world), IndexFilePartialList (stored neither 0 nor count),
// IndexFileTruncated.
template <class Read>
IndexFileHeader read_index_file_header(Read&& read, uint64_t size) {
    unsigned char b[IndexFileHeader::kShardBytes];
    index_file_advance(0, 1, IndexFileHeader::kMagicBytes, size);
    read(uint64_t(0), (void*)b, (size_t)IndexFileHeader::kMagicBytes);
    const uint64_t n = IndexFileHeader::shard_magic(b) ? IndexFileHeader::kShardBytes : IndexFileHeader::kIndexBytes;
    index_file_advance(0, 1, n, size);
    read(IndexFileHeader::kMagicBytes, (void*)(b + IndexFileHeader::kMagicBytes), (size_t)(n - IndexFileHeader::kMagicBytes));
    return IndexFileHeader::decode(b);
}

template <class Read>
IndexFileDirectory read_index_file_lists(const IndexFileHeader& h, Read&& read, uint64_t size) {
    if (h.shard && (h.world == 0 || h.rank >= h.world)) throw IndexFileBadShard();
    IndexFileDirectory d;
    d.header = h;
    d.centroids_off = h.bytes();
    uint64_t at = index_file_advance(d.centroids_off, h.nlist, h.row_bytes(), size);
    index_file_advance(at, h.nlist, h.list_header_bytes(), size);  // (nlist itself, before it sizes anything)
    d.lists.resize(h.nlist);
    for (IndexFileDirectory::List& l : d.lists) {
        uint64_t w[2] = {0, 0};
        l.ids_off = index_file_advance(at, 1, h.list_header_bytes(), size);
        read(at, (void*)w, (size_t)h.list_header_bytes());
        l.count = w[0];
        l.stored = h.shard ? w[1] : w[0];
        if (l.stored != 0 && l.stored != l.count) throw IndexFilePartialList();
        at = index_file_advance(l.ids_off, l.stored, IndexFileHeader::kIdBytes + h.row_bytes(), size);
    }
    d.end = at;
    return d;
}

template <class Read>
IndexFileDirectory read_index_file(Read&& read, uint64_t size) {
    return read_index_file_lists(read_index_file_header(read, size), read, size);
}

// The writer's two steps over put(bytes, n): the header with the centroids, then one list's
// record (`stored` of its `count` rows: all or none).
template <class Put>
void write_index_file_head(const IndexFileHeader& h, const float* centroids, Put&& put) {
    unsigned char b[IndexFileHeader::kShardBytes];
    h.encode(b);
    put((const void*)b, (size_t)h.bytes());
    put((const void*)centroids, (size_t)((uint64_t)h.nlist * h.row_bytes()));
}

template <class Put>
void write_index_file_list(const IndexFileHeader& h, uint64_t count, uint64_t stored, const uint64_t* ids,
                           const float* vectors, Put&& put) {
    put((const void*)&count, (size_t)IndexFileHeader::kIdBytes);
    if (h.shard) put((const void*)&stored, (size_t)IndexFileHeader::kIdBytes);
    put((const void*)ids, (size_t)(stored * IndexFileHeader::kIdBytes));
    put((const void*)vectors, (size_t)(stored * h.row_bytes()));
}

}  // namespace vdbe
