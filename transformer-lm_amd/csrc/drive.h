// Host driver of train_bpe(path) (drive.hip): parallel file -> HBM staging, slab cutting and
// the multi-device trainer.
#pragma once

#include <string>
#include <vector>

#include "internal.h"

namespace bpe {

// Bytes of a corpus: a regular file (read with pread by many threads) or host memory (a pipe
// or FIFO is read to EOF first).
struct Source {
    int fd = -1;
    const uint8_t* mem = nullptr;
    size_t size = 0;
    std::string name;
    std::vector<uint8_t> owned;
    static Source open_path(const char* path);   // throws Error{BPE_E_IO} with errno
    static Source memory(const uint8_t* p, size_t n);
    Source() = default;
    Source(Source&& o) noexcept
        : fd(o.fd), mem(o.mem), size(o.size), name(std::move(o.name)), owned(std::move(o.owned)) {
        o.fd = -1;
        if (!owned.empty()) mem = owned.data();
    }
    Source(const Source&) = delete;
    ~Source();
    void read(size_t off, size_t len, uint8_t* dst) const;
};

int io_threads();
// g + 1 cut points [0, c1, ..., size] at safe split points
std::vector<size_t> slab_cuts(const Source& src, int g);
// src[off, off + len) -> d_dst on `device`, through pinned staging, `threads` readers
void stage_to_device(const Source& src, size_t off, size_t len, uint8_t* d_dst, int device, int threads);
// d_src[0, len) on `device` -> host memory h_dst (pageable), through pinned staging, `threads` copiers
void device_to_host(const uint8_t* d_src, size_t len, uint8_t* h_dst, int device, int threads);
// src[off, off + len) -> d_dst, validated and counted segment by segment as it arrives
// (false: the text holds a \r, so the caller must apply universal newlines and count it whole).
// min_cap: a lower bound (a power of two) for the word table's slots, when the caller knows
// better than the size rule of the whole-corpus count (windows: counter_add_source)
bool load_and_count(const Source& src, size_t off, size_t len, uint8_t* d_dst, int device, int threads,
                    hipStream_t stream, Prepared& pre, size_t min_cap = 0);
std::vector<int> pick_devices(int n_gpus);
// train_bpe over the whole source on n_gpus devices of this process (<= 0: all visible)
void train_source(const Source& src, int vocab_size, const std::vector<std::string>& specials, int n_gpus,
                  TrainOutput& out);
// one rank of a multi-process job: the source is this rank's slab, or (split) the whole corpus
// of which this rank reads its share
void train_source_comm(const Source& src, bool split, int vocab_size, const std::vector<std::string>& specials,
                       Comm* comm, TrainOutput& out);
// One document into a word accumulator without holding more than one window of it in HBM: the
// source is cut into windows of about window_bytes (0: kDefaultWindow; at least 64 KiB) at safe
// split points, each window is loaded, validated and counted into one reused corpus buffer and
// folded.  All or nothing: after an error `acc` holds what it held before.  A UTF-8 error names
// the byte's position in the source.
// The default is a choice, not a measured optimum: 8 GiB of text plus the counter's scratch
// (about 4 bytes per byte) is about 40 GB of HBM.
constexpr size_t kDefaultWindow = (size_t)8 << 30;
// errors (BPE_UTF8_*): 0 is strict.  In mode 1 or 2 a window whose validation fails is repaired
// where it lies in HBM (utf8fix.hip) and counted again; report (may be NULL) gets what was
// repaired, its first position relative to the source.
void counter_add_source(WordAccumulator& acc, const Source& src, size_t window_bytes, int errors = 0,
                        bpe_utf8_stats* report = nullptr);
// the same for raw bytes already in device memory (one window; d_data is not modified)
void counter_add_device(WordAccumulator& acc, const uint8_t* d_data, size_t n, hipStream_t stream, int errors = 0,
                        bpe_utf8_stats* report = nullptr);
// bpe_release_device_memory: the corpus buffers kept for `dev` (< 0: every device) go back to the
// device allocator; returns the bytes freed.  Buffers a running call holds are not touched, and the
// cached copy streams are kept for the process (a concurrent transfer may be using them)
size_t corpus_release(int dev);

}  // namespace bpe
