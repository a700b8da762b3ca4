// Host-side interfaces shared by the libbpe355 translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "bpe_common.h"

namespace bpe {

// ---------------------------------------------------------------- communicator
// Sum-all-reduce of int64 buffers across the ranks that each own one corpus slab.
struct Comm {
    int nranks = 1, rank = 0, device = 0;
    virtual ~Comm() = default;
    // in-place sum over ranks of d_buf[0..count) (device memory), ordered on `stream`
    virtual void allreduce_i64(int64_t* d_buf, size_t count, hipStream_t stream) = 0;
    // d_recv[r * bytes .. (r + 1) * bytes) = rank r's d_send[0 .. bytes) (default: through
    // allreduce_i64; RCCL overrides it with ncclAllGather)
    virtual void allgather_bytes(const void* d_send, size_t bytes, void* d_recv, hipStream_t stream);
    // all-to-all of variable sizes: rank p receives scnt[p] bytes from d_send + soff[p] of this
    // rank, and this rank's d_recv + roff[q] gets rcnt[q] bytes from rank q (default: through
    // allgather_bytes, every rank's whole send buffer; RCCL and the in-process ranks override it
    // with point-to-point copies)
    virtual void alltoallv_bytes(const void* d_send, const size_t* soff, const size_t* scnt, void* d_recv,
                                 const size_t* roff, const size_t* rcnt, hipStream_t stream);
};

// ---------------------------------------------------------------- small transfers (hostio.hip)
// host <- device and device <- host through a pinned device-mapped buffer moved by a kernel (no
// copy-engine queue, so they do not wait behind bulk DMA); return once the bytes have arrived
void to_host(void* dst, const void* d_src, size_t bytes, hipStream_t stream);
void to_device(void* d_dst, const void* src, size_t bytes, hipStream_t stream);

// ---------------------------------------------------------------- text preparation
// Validates strict UTF-8 and applies universal newlines (reference train.py:22 text-mode
// read).  Returns the device pointer to use (d_in itself when no \r is present, else
// `scratch`) and the resulting length.  Throws Error{BPE_E_UTF8} on bad input.
const uint8_t* prepare_text(const uint8_t* d_in, size_t n, DevBuf<uint8_t>& scratch,
                            size_t* n_out, hipStream_t stream);

// Byte offsets of characters 0, k, 2k, ... of the UTF-8 text d_text[0, n) (io.hip): where the
// pieces f.read(k) returns begin (reference encode.py:31-33).
std::vector<uint64_t> utf8_piece_starts(const uint8_t* d_text, size_t n, size_t k, hipStream_t stream);
// The same over a range of a longer text whose first character is character c_base: appends the
// starts found (plus `offset`) to out, returns the range's character count.  scratch (optional)
// keeps the device arrays across calls: a freed device buffer synchronises the whole device, which
// in the overlapped encode_file would wait for the copies other threads have in flight.
struct PieceScratch {
    DevBuf<unsigned long long> cnt, first, marks;
    DevBuf<uint8_t> tmp;
};
uint64_t piece_starts_range(const uint8_t* d_text, size_t n, size_t k, uint64_t c_base, uint64_t offset,
                            hipStream_t stream, std::vector<uint64_t>& out, PieceScratch* scratch = nullptr);

// ---------------------------------------------------------------- id stream statistics (idstats.hip)
// Ids of elem_bytes 2, 4 or 8 in device memory, aligned to their own size only.  Both calls return
// once their result is complete; scratch keeps the device arrays across calls.
struct IdScratch {
    DevBuf<unsigned long long> blk_cnt, blk_off, flags;
    DevBuf<uint8_t> tmp;
};
// d_counts[id] += occurrences (64-bit).  An id at or above n_counts: Error{BPE_E_ARG} naming the
// smallest one, and the table is then not to be used.
void ids_histogram(const void* d_ids, size_t n, int elem_bytes, unsigned long long* d_counts, size_t n_counts,
                   hipStream_t stream, IdScratch& scratch);
// base + i for every i with ids[i] == value, ascending, the first `cap` of them into d_pos; returns
// how many there are (more than cap: call again with room for all)
size_t ids_find(const void* d_ids, size_t n, int elem_bytes, uint64_t value, uint64_t base, unsigned long long* d_pos,
                size_t cap, hipStream_t stream, IdScratch& scratch);

// ---------------------------------------------------------------- unique-word count
struct WordCounts {
    DevBuf<unsigned long long> kv;    // cap x {key, count} (layout: text.hip), key 0 = empty
    DevBuf<unsigned long long> pos;   // cap: an occurrence of each inline-keyed word
    size_t cap = 0;
    uint64_t n_pretokens = 0;         // multi-byte pre-tokens seen
    uint64_t n_records = 0;           // cache misses spilled as records (count.hip)
    double reduce_ms = 0;             // device time of their aggregation after the last launch (when timed)
    double partial_ms = 0;            // ... and of the batches aggregated between launches (file path)
    unsigned batches = 0;             // aggregation batches
};
// Pre-tokenize text[0..n) with the GPT-2 pattern and count the multi-byte words.
// (Single-byte words carry no pairs and cannot affect training.)
void count_words(const uint8_t* d_text, size_t n, WordCounts& wc, hipStream_t stream,
                 float* kernel_ms);

// The same count over a text that arrives in segments [lo, hi) cut at safe split points
// (text.hip): range() enqueues one launch per segment into one table; finish() returns false
// when the table overflowed (then recount everything with a larger table).
struct RecPoolOwner;
struct CountPass {
    WordCounts wc;
    bool v2 = true;                       // the byte-parallel counter (count.hip); BPE355_COUNT_V1: the serial one
    std::unique_ptr<RecPoolOwner> rec;    // its record pool (large texts)
    bool pool_fallback = false;           // the pool did not fit in device memory: misses go to the table
    unsigned grid2 = 0;
    DevBuf<unsigned> status;
    DevBuf<unsigned long long> ntok, fill;
    const uint8_t* text = nullptr;
    size_t total = 0;
    hipStream_t s = nullptr;
    bool timed = false;
    const unsigned long long* gate = nullptr;   // device flag: skip the launches unless ~0
    double kernel_ms = 0;        // summed device time of the launches (when timed)
    std::vector<hipEvent_t> ev, pev;   // count launches, partial aggregations
    static size_t initial_cap(size_t n);
    void begin(const uint8_t* d_text, size_t n, size_t cap, hipStream_t stream, bool timing);
    void range(size_t lo, size_t hi);
    // aggregate the records of the pages completed so far (the file path calls it between
    // segments, while the next ones arrive); finish() does the rest
    void partial();
    bool finish();
    CountPass();
    ~CountPass();
};

// Strict UTF-8 validation by segment (the first bad byte, and whether any \r is present).
struct ValidatePass {
    DevBuf<unsigned long long> flags;
    const uint8_t* text = nullptr;
    size_t total = 0;
    hipStream_t s = nullptr;
    void begin(const uint8_t* d_text, size_t n, hipStream_t stream);
    void range(size_t lo, size_t hi);
    // the units not yet validated whose windows lie inside the loaded prefix [0, loaded) of a
    // text that ends at `total` (all of them once loaded == total); returns the validated end
    size_t prefix(size_t loaded);
    size_t done_units = 0;
    void finish(unsigned long long* err_pos, bool* has_cr);   // err_pos ~0: none
};

// A corpus already validated and counted (the overlapped file path, drive.hip)
struct Prepared {
    const uint8_t* text = nullptr;
    size_t n = 0;
    WordCounts wc;
    double t_prepare_ms = 0, t_count_ms = 0, load_ms = 0;
    float count_kernel_ms = 0;
};

// ---------------------------------------------------------------- multi-GPU word exchange
// Replace this rank's word table by the union of every rank's (counts summed), whose words'
// bytes live in `all` (exchange.hip).  One all-gather; afterwards no rank needs the others.
// stats (may be null): t_gather_ms, t_union_ms and exchange_seg_bytes are filled in.
void union_word_tables(const uint8_t* text, WordCounts& wc, Comm* comm, hipStream_t stream,
                       DevBuf<uint8_t>& all, uint64_t* union_words, bpe_train_stats* stats = nullptr);

// ---------------------------------------------------------------- training driver
struct TrainOutput {
    std::vector<std::pair<uint32_t, uint32_t>> merges_internal;  // (a, b) internal ids
    std::vector<std::string> tok_bytes;                          // internal id -> bytes
    std::vector<std::pair<std::string, std::string>> merges;     // byte pairs, in order
    bpe_train_stats stats{};
};
struct TrainOpts {
    size_t slab_offset = 0;     // this slab's first byte in the whole corpus (error positions)
    bool merge_loop = true;     // false: stop after the word exchange (another rank trains)
    bool has_pending = false;   // an error this rank hit before training (e.g. reading its
    Error pending{0, ""};       // slab); raised by every rank together, before any collective
};
std::unique_ptr<Comm> make_rccl_comm(const uint8_t id[128], int nranks, int rank, int device);
// ranks that are threads of one process, possibly sharing a device (tests; comm.hip)
std::shared_ptr<void> make_inproc_group();
std::unique_ptr<Comm> make_inproc_comm(const std::shared_ptr<void>& group, int nranks, int rank, int device);
// BPE355_EXCHANGE=rounds: several ranks keep their slabs' words and all-reduce the pair deltas
// every round, so every rank runs the merge loop (default: one word-table exchange)
bool per_round_exchange();
void train_on_device(const uint8_t* d_raw, size_t n, int vocab_size,
                     const std::vector<std::string>& specials, Comm* comm, hipStream_t stream,
                     TrainOutput& out, const TrainOpts& opt = TrainOpts{}, Prepared* pre = nullptr);

// The merge loop on a word table whose words' bytes live in `text` (the corpus, a gathered buffer,
// an accumulator's pool): base vocab, rounds, word build, merges into `out`; nothing when
// vocab_size is not above the base vocab (merge_rounds <= 0).  The table is read, never changed;
// drop_after_build (may be null) is released once the loop holds its own copy of the words.
long long merge_rounds(int vocab_size, const std::vector<std::string>& specials);
void train_words(const uint8_t* text, const WordCounts& wc, int vocab_size, const std::vector<std::string>& specials,
                 hipStream_t stream, TrainOutput& out, Comm* loop_comm = nullptr,
                 WordCounts* drop_after_build = nullptr);

// ---------------------------------------------------------------- word accumulator (accum.hip)
// A word table that owns its bytes and sums counts over many inputs: the {key, count} + pos
// table of WordCounts over an append-only byte pool, which is the table's "text" (keys of words
// longer than 7 bytes are len << 40 | pool offset + 1, pos[] of an inline word is its pool
// offset).  One device (the one current at creation), one caller at a time.  Ranks of a larger
// job can each count their shards and absorb one another's exported words (export_words ->
// add_records).
// Limits (BPE_E_LIMIT, never wrapped): a word of kMaxPretok bytes or more; pool offsets past
// 2^40 - 2; 2^31 distinct words; and the sum over all words of count x length at 2^62 or more
// -- the merge loop's pair counters are signed 64-bit (train.hip, PairsDev::cnt), and no pair
// can occur more often than that sum.  The last is checked when words are added from records
// and again at train().
struct AccumInfo {
    uint64_t n_words = 0, n_pretokens = 0, n_bytes = 0, n_inputs = 0, n_windows = 0, max_window_bytes = 0;
    uint64_t table_slots = 0, pool_bytes = 0, pool_live_bytes = 0, n_grows = 0;
    double t_load_ms = 0, t_count_ms = 0, t_fold_ms = 0;
};
class WordAccumulator {
   public:
    WordAccumulator();    // on the current device; BPE355_ACC_SLOTS / BPE355_ACC_POOL: initial sizes (tests)
    ~WordAccumulator();
    WordAccumulator(const WordAccumulator&) = delete;
    WordAccumulator& operator=(const WordAccumulator&) = delete;
    int device() const { return dev_; }
    hipStream_t stream() const { return s_; }
    // every word of a shard's table (bytes in `text`), counts summed; returns once `text` and
    // `wc` are no longer needed.  weight: an upper bound of the shard's sum of count x length
    // (its byte count).  Returns the shard's distinct words.
    size_t fold(const uint8_t* text, const WordCounts& wc, uint64_t weight);
    // the most distinct words any folded shard held: sizes the next window's count table
    size_t shard_words_hint() const { return shard_words_; }
    // (u32 len, bytes, u64 count) records in host memory; words under 2 bytes and zero counts are
    // dropped.  A truncated blob: BPE_E_ARG, nothing added
    void add_records(const uint8_t* blob, size_t n);
    void absorb(const WordAccumulator& o);   // o unchanged; same device
    // the words not equal to a special as (u32 len, bytes, u64 count) records, malloc'ed
    void export_words(const std::vector<std::string>& specials, uint8_t** blob, size_t* blob_n) const;
    void train(int vocab_size, const std::vector<std::string>& specials, TrainOutput& out) const;
    void clear();
    AccumInfo info() const;
    // bookkeeping of the inputs (drive.hip): one add_* call, its windows, its timings
    void note_input(uint64_t n_bytes, uint64_t n_windows, uint64_t max_window, double load_ms, double count_ms);

   private:
    struct Scratch;
    void fold_list(const uint8_t* text, const unsigned long long* w_off, const uint32_t* w_len,
                   const unsigned long long* w_cnt, size_t n);
    size_t list_table(const unsigned long long* kv, const unsigned long long* pos, size_t cap, const uint8_t* text,
                      const std::vector<std::string>& specials) const;
    void ensure(size_t n_new, size_t new_bytes);
    int dev_ = 0;
    hipStream_t s_ = nullptr;
    WordCounts wc_;              // kv, pos, cap (n_pretokens: the accumulated count)
    DevBuf<uint8_t> pool_;       // (+ 16 bytes of padding past pool_cap_)
    size_t pool_cap_ = 0, pool_used_ = 0, n_words_ = 0, shard_words_ = 0;
    uint64_t weight_ = 0;        // upper bound of sum(count x length), saturating
    AccumInfo st_;
    std::unique_ptr<Scratch> sc_;   // grow-only device arrays of the folds and exports
};

bool timing_enabled();

// ---------------------------------------------------------------- encode with dropout (dropout.hip)
// BPE-dropout draws per occurrence, so nothing of the encoder behind its scan applies: encode.hip
// runs its front (the segment table and the scan's kCuts, kPos instantiation) and hands the
// records to dropout_emit, which merges every pre-token occurrence on its own.
struct DropParams {
    uint32_t thr;               // a candidate merge is skipped when its 24-bit draw is below thr
    uint64_t seed, doc_base;    // document i of the call draws with doc_key = doc_base + i
};
struct DropTables {             // the tokenizer's tables (EncTables of encode.hip)
    const unsigned long long* pm_key;  // ((a << 32) | b) + 1
    const uint2* pm_val;               // (rank, product)
    unsigned long long pm_mask;
    const int64_t* tok2vid;            // internal token -> vocab id, -1 if absent
    const uint32_t* byte2tok;
    const uint8_t* sp_bytes;
    const uint32_t* sp_off;
    const uint32_t* sp_len;
    const int64_t* sp_vid;
    int n_sp;
};
struct DropFront {              // what the scan left, all device memory unless noted
    const uint8_t* text;
    size_t n, n_chunks, chunk;  // chunk: the bytes of one (kChunk)
    uint32_t* recs;             // per record: its kind (only "special k" is read); reused for its id count
    uint32_t kind_mask, kind_special, payload_mask;
    const uint16_t* rec_pos;    // per record: its first byte, relative to its chunk
    const unsigned long long* rec_base;   // per chunk: its run in recs / rec_pos
    const uint32_t* rec_n;
    const unsigned long long* chunk_next; // per chunk: the end of its last record
    const unsigned long long* cuts;       // the document starts inside the text: sorted, distinct
    const uint32_t* chunk_cut0;           // n_chunks + 1: the first cut at or after each chunk's first byte
    const uint32_t* cut_rec;              // per cut: the record that starts there, inside its chunk's run
    const std::vector<unsigned long long>* h_cuts;   // host: the cuts
    const uint64_t* h_doc_starts;         // host
    size_t n_docs;
    uint32_t* d_ids;                      // out: >= n ids
    unsigned long long* d_id_offsets;     // out: n_docs + 1
};
struct DropScratch {            // kept by the tokenizer between calls (grow-only)
    DevBuf<uint32_t> pool, doc_cut;
    DevBuf<unsigned long long> ctot, coff, cut_off, cut_doc, list;
    DevBuf<unsigned> status;
    DevBuf<uint8_t> tmp;
};
// returns the id count once d_ids and d_id_offsets are written
size_t dropout_emit(const DropFront& F, const DropTables& E, const DropParams& P, DropScratch& S, hipStream_t s);
// encode.hip: the front and dropout_emit for one batch (the document starts are checked as
// bpe_tok_encode_batch checks them); s null: the tokenizer's own stream
size_t encode_dropout_device(bpe_tokenizer* tok, const uint8_t* d_text, size_t n, const uint64_t* doc_starts,
                             size_t n_docs, const DropParams& P, uint32_t* d_ids, unsigned long long* d_id_offsets,
                             hipStream_t s);
hipStream_t tokenizer_stream(bpe_tokenizer* tok);

}  // namespace bpe
