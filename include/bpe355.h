/*
 * libbpe355 -- MI355X (gfx950) byte-level BPE trainer and encoder, C ABI.
 *
 * The drop-in boundary for gashon/transformer-lm's tokenizer path.  The reference has no
 * FFI (it is pure Python); these entry points are what its two Python APIs bind to through
 * ctypes (binding: transformer-lm_amd/bpe_amd/_lib.py):
 *
 *   bpe_train_file / bpe_train_buffer   <- train_bpe(input_path, vocab_size, special_tokens)
 *                                          reference models/tokenizer/train.py:142-231 (its
 *                                          OWT caller, perf/bpe/util.py:16, is one process:
 *                                          n_gpus spreads that one call over the node's GPUs)
 *   bpe_tok_create                      <- Tokenizer.__init__(vocab, merges, special_tokens)
 *                                          reference models/tokenizer/tokenizer.py:12-38
 *   bpe_tok_encode                      <- Tokenizer.encode(text)
 *                                          reference models/tokenizer/tokenizer.py:111-138
 *
 * Conventions
 *  - Every function returns 0 (BPE_OK) or a negative BPE_E_* code; bpe_last_error() gives the
 *    message of the calling thread's last failure.  The Python binding maps BPE_E_IO to
 *    OSError/FileNotFoundError, BPE_E_UTF8 to UnicodeDecodeError and BPE_E_KEY to KeyError,
 *    the exception types the reference raises (train.py:22, tokenizer.py:135).
 *  - Plain pointers and sizes only.  The library owns result objects until *_free().
 *  - Byte-string lists cross the boundary as blobs: a sequence of (u32 little-endian length,
 *    bytes) records.  Merges: (len a, a, len b, b) per merge, in creation order.  Vocab:
 *    (len, bytes) per id, ids 0..n-1 in order (reference Vocab ids are dense, vocab.py:32).
 *  - There is no CPU fallback: without a usable gfx950 device every compute call fails with
 *    BPE_E_HIP.
 */
#ifndef BPE355_H
#define BPE355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPE355_ABI_VERSION 2

enum {
    BPE_OK = 0,
    BPE_E_IO = -1,       /* file could not be read (errno in bpe_last_errno()) */
    BPE_E_UTF8 = -2,     /* input is not valid UTF-8 (reference: UnicodeDecodeError) */
    BPE_E_KEY = -3,      /* a merged token is missing from the vocab (reference: KeyError) */
    BPE_E_HIP = -4,      /* HIP runtime / device failure, or no gfx950 device */
    BPE_E_ARG = -5,      /* invalid argument */
    BPE_E_NOMEM = -6,    /* device or host allocation failed */
    BPE_E_RCCL = -7,     /* collective failure */
    BPE_E_LIMIT = -8     /* input exceeds a documented limit (pre-token >= 8 MiB, corpus > 1 TiB) */
};

typedef struct bpe_result bpe_result;
typedef struct bpe_tokenizer bpe_tokenizer;
typedef struct bpe_comm bpe_comm;

int bpe_abi_version(void);
/* The HIP runtime this process bound the library to.  The library is compiled against the ROCm
 * headers of the build image (HIP_VERSION, *compiled); the libamdhip64.so.7 that serves it is
 * whichever copy of that soname the process loaded first -- inside a PyTorch-ROCm process,
 * torch's bundled one (*runtime, hipRuntimeGetVersion; runtime_path: the file, via dladdr).
 * The Python binding refuses a runtime of a different major version. */
int bpe_runtime_info(int* compiled_hip_version, int* runtime_hip_version, char* runtime_path, size_t cap);
const char* bpe_last_error(void);
int bpe_last_errno(void);
/* number of visible gfx950 devices (0 if none); never fails */
int bpe_device_count(void);

/* ---------------------------------------------------------------- multi-GPU (RCCL) */
/* One process per GPU.  Rank 0 creates the id, the caller broadcasts its 128 bytes (e.g. with
 * torch.distributed), every rank calls bpe_comm_init.  A NULL comm means single GPU. */
int bpe_comm_unique_id(uint8_t id_out[128]);
int bpe_comm_init(const uint8_t id[128], int nranks, int rank, int device, bpe_comm** out);
/* A host-staged communicator for testing the sharded path without RCCL: the library calls
 * fn(ctx, buf, count) to all-reduce `count` int64 values in place (sum) on the host. */
typedef int (*bpe_host_allreduce_fn)(void* ctx, int64_t* buf, size_t count);
int bpe_comm_init_host(bpe_host_allreduce_fn fn, void* ctx, int nranks, int rank, int device,
                       bpe_comm** out);
void bpe_comm_free(bpe_comm* comm);

/* ---------------------------------------------------------------- training */
/* train_bpe(input_path, vocab_size, special_tokens) (reference train.py:142-231): reads the
 * file like the reference's open(path, "r", encoding="utf-8").read() (train.py:22: strict
 * UTF-8, universal newlines; a pipe or FIFO is read to EOF).  The file is read by a pool of
 * host threads into pinned staging and copied to HBM while the next piece is read.
 * n_gpus: devices of THIS process to use (<= 0: every visible device).  With more than one,
 * each device takes one slab of the file cut at safe split points, counts its words, one RCCL
 * all-gather merges the word tables and the first device trains on the union.  The result is
 * identical for every n_gpus.  Errors: BPE_E_IO (errno: ENOENT, EISDIR, ...), BPE_E_UTF8. */
int bpe_train_file(const char* path, int vocab_size, const char* const* specials, int n_specials,
                   int n_gpus, bpe_result** out);
/* One rank of a multi-process job (one process per GPU, comm from bpe_comm_init):
 * split = 0: the file is this rank's slab (slabs cut at pre-token boundaries, bpe_safe_split);
 * split = 1: the file is the whole corpus and this rank reads its share of it.
 * All ranks obtain the identical, global result. */
int bpe_train_file_comm(const char* path, int vocab_size, const char* const* specials,
                        int n_specials, bpe_comm* comm, int split, bpe_result** out);
/* train_bpe on raw file bytes in host memory (this rank's slab when comm is set) */
int bpe_train_buffer(const uint8_t* data, size_t n, int vocab_size, const char* const* specials,
                     int n_specials, bpe_comm* comm, bpe_result** out);
/* same, spread over n_gpus devices of this process as bpe_train_file does */
int bpe_train_buffer_gpus(const uint8_t* data, size_t n, int vocab_size,
                          const char* const* specials, int n_specials, int n_gpus,
                          bpe_result** out);
/* same, raw bytes already resident in device memory (d_data on the current device; it is not
 * modified).  stream may be NULL (the library's own stream). */
int bpe_train_device(const uint8_t* d_data, size_t n, int vocab_size, const char* const* specials,
                     int n_specials, bpe_comm* comm, void* hip_stream, bpe_result** out);

/* extract_subword_frequencies (reference train.py:16-28) on the device, for checking the
 * pre-tokenizer + counter on its own: the multi-byte pre-tokens of the text-mode-decoded
 * bytes and their counts (1-byte words carry no pairs and are not counted; pre-tokens equal to
 * a special are skipped, train.py:25).  *blob: (u32 len, bytes, u64 count) records in no
 * particular order, malloc'ed; release with bpe_blob_free. */
int bpe_word_counts(const uint8_t* data, size_t n, const char* const* specials, int n_specials,
                    uint8_t** blob, size_t* blob_n);
void bpe_blob_free(uint8_t* blob);

int64_t bpe_result_n_merges(const bpe_result* r);
int64_t bpe_result_n_vocab(const bpe_result* r);
/* blob views owned by the result */
size_t bpe_result_merges_blob(const bpe_result* r, const uint8_t** data);
size_t bpe_result_vocab_blob(const bpe_result* r, const uint8_t** data);
/* The same records flat: which = 0 merges (a0, b0, a1, b1, ...), 1 vocab in id order; *lens gets
 * one length per record, *bytes their concatenation (*n_bytes long); returns the record count.
 * (Host-side plumbing for the Python shim: one buffer sliced, not one parse per record.) */
size_t bpe_result_flat(const bpe_result* r, int which, const uint32_t** lens, const uint8_t** bytes,
                       size_t* n_bytes);
/* The merges as vocab ids: *ids gets (a0, b0, a1, b1, ...), the ids of flat record order 1 whose
 * bytes each merge joins; returns the merge count (0: not available, use bpe_result_flat 0).  The
 * Python shim then builds merges from the vocab's own bytes objects, as the reference does when it
 * appends (vocab[a], vocab[b]) (train.py:191-196), instead of one new bytes object per part. */
size_t bpe_result_merge_ids(const bpe_result* r, const uint32_t** ids);

typedef struct {
    double t_total_ms;        /* whole call, host wall clock */
    double t_prepare_ms;      /* UTF-8 check + newline translation */
    double t_count_ms;        /* pre-tokenize + unique-word count */
    double t_words_ms;        /* word table + initial pair histogram */
    double t_merge_ms;        /* merge loop */
    double merge_kernel_ms;   /* summed device time of the merge-apply kernel (event-timed) */
    int64_t merge_kernel_launches;
    double merge_kernel_bytes; /* algorithmic bytes moved by those launches */
    double count_kernel_ms;   /* device time of the pre-tokenize/count kernel */
    double count_kernel_bytes;
    int64_t n_bytes;          /* corpus bytes after newline translation (this rank) */
    int64_t n_pretokens;      /* pre-tokens counted (this rank, excl. 1-byte and specials) */
    int64_t n_words;          /* unique multi-byte words (this rank) */
    int64_t n_word_tokens;    /* initial token slots over those words */
    int64_t n_pairs_final;    /* pair-table keys at the end */
    int64_t n_rebuilds;       /* candidate-set rebuilds */
    int64_t n_rounds_device;  /* merges decided on the device */
    int64_t n_rounds_host;    /* zero-count merges emitted after exhaustion */
    int64_t n_index_builds;   /* word-table compactions + posting-list builds */
    int64_t n_trips;          /* merge-loop round trips (several exact merges each when batched) */
    int64_t n_rounds_batched; /* rounds taken in trips of more than one merge */
    double t_exchange_ms;     /* multi-GPU word-table exchange (0 on one rank) */
    int64_t n_exchanged_words; /* local unique words of all ranks gathered (before dedupe) */
    double t_load_ms;         /* file / host buffer -> HBM (0 when the corpus starts in HBM) */
    int64_t n_gpus;           /* devices (ranks) that took part */
    double count_reduce_ms;   /* device time aggregating the counter's spilled records */
    int64_t n_count_records;  /* pre-tokens (or cache entries) spilled as records by the counter */
    double count_partial_ms;  /* device time of the aggregations done while the file was loading */
    int64_t n_count_batches;  /* aggregation batches (1 + those done during the load) */
    double t_gather_ms;       /* multi-GPU word exchange: the all-gather of the segments */
    double t_union_ms;        /* multi-GPU word exchange: the union-table inserts */
    int64_t exchange_seg_bytes; /* multi-GPU word exchange: one rank's segment (all ranks' equal) */
    double t_alltoall_ms;     /* multi-GPU word exchange: the all-to-all of the words by owner */
    double t_owner_ms;        /* multi-GPU word exchange: the owner-table inserts */
    int64_t exchange_a2a_bytes; /* multi-GPU word exchange: the bytes this rank sent in the all-to-all */
} bpe_train_stats;
int bpe_result_stats(const bpe_result* r, bpe_train_stats* out);
void bpe_result_free(bpe_result* r);

/* ---------------------------------------------------------------- word counter */
/* A device-resident {pre-token -> count} table that accumulates over many inputs and can be
 * trained on: many files, a file larger than HBM (counted window by window), pre-counted words,
 * several vocab sizes or special-token lists from one count.  The reference's trainer sees its
 * corpus only through that multiset (train.py:16-49), so the result is bit-identical to training
 * on the inputs as the reference would see them.
 *  - Each bpe_counter_add_* call is one document: its pre-tokens end at its ends, exactly as a
 *    separate extract_subword_frequencies (train.py:16-28) on that input would have them.
 *  - The counter is independent of special tokens: it keeps every multi-byte pre-token, and
 *    bpe_counter_words / bpe_counter_train leave out the words equal to a special (train.py:25).
 *  - Training reads the counter and leaves it as it was: add more and train again.
 *  - One device: the one current at bpe_counter_create.  The ranks of a larger job can each
 *    count their shards, export them with bpe_counter_words and bpe_counter_add_words them into
 *    one counter.  Calls of several threads on one counter take turns; different counters run
 *    side by side.
 *  - Limits (BPE_E_LIMIT, nothing wraps): a pre-token of 8 MiB or more; 2^40 bytes of distinct
 *    words; 2^31 distinct words; the sum over all words of count x length at 2^62 or more (the
 *    merge loop counts pairs in signed 64-bit integers), checked by bpe_counter_add_words,
 *    bpe_counter_absorb and bpe_counter_train. */
typedef struct bpe_counter bpe_counter;
typedef struct {
    uint64_t n_words;           /* distinct multi-byte pre-tokens held */
    uint64_t n_pretokens;       /* their summed counts */
    uint64_t n_bytes;           /* text bytes counted (after newline translation; none for add_words) */
    uint64_t n_inputs;          /* bpe_counter_add_* calls that succeeded */
    uint64_t n_windows;         /* windows those inputs were counted in */
    uint64_t max_window_bytes;  /* the longest of them */
    uint64_t table_slots;       /* slots of the word table (load <= 1/2) */
    uint64_t pool_bytes;        /* capacity of the byte pool that holds the words */
    uint64_t pool_live_bytes;   /* bytes of it that words occupy (a word's bytes are stored once) */
    uint64_t n_grows;           /* table rehashes and pool reallocations so far */
    double t_fold_ms;           /* host time spent merging counted tables into the counter */
} bpe_counter_info_t;
int bpe_counter_create(bpe_counter** out);
/* The file at path as bpe_train_file reads it (strict UTF-8, universal newlines; BPE_E_IO,
 * BPE_E_UTF8 with the byte's position in the file), counted in windows of about window_bytes
 * (0: the default, 8 GiB -- a choice, not a measured optimum; at least 64 KiB) cut at safe split
 * points, so that HBM holds one window (plus about 4 bytes of scratch per byte) at a time.  All or
 * nothing: after an error the counter holds what it held before. */
int bpe_counter_add_file(bpe_counter* c, const char* path, size_t window_bytes);
/* raw file bytes in host memory: one document */
int bpe_counter_add_buffer(bpe_counter* c, const uint8_t* data, size_t n);
/* the same, bytes in device memory on the counter's device (not modified); stream may be NULL */
int bpe_counter_add_device(bpe_counter* c, const uint8_t* d_data, size_t n, void* hip_stream);
/* (u32 len, bytes, u64 count) records as bpe_word_counts and bpe_counter_words return them; words
 * under 2 bytes are dropped, equal words summed.  A truncated blob: BPE_E_ARG, counter unchanged. */
int bpe_counter_add_words(bpe_counter* c, const uint8_t* blob, size_t blob_n);
/* dst += src; src is unchanged; both on one device */
int bpe_counter_absorb(bpe_counter* dst, const bpe_counter* src);
/* The words not equal to a special and their counts, packed on the device and copied out once:
 * (u32 len, bytes, u64 count) records in no particular order; release with bpe_blob_free. */
int bpe_counter_words(const bpe_counter* c, const char* const* specials, int n_specials, uint8_t** blob,
                      size_t* blob_n);
/* train_bpe on the counted words.  The stats carry the accumulated n_bytes and n_pretokens,
 * t_load_ms and t_count_ms summed over the add calls, and the training's own fields as usual. */
int bpe_counter_train(const bpe_counter* c, int vocab_size, const char* const* specials, int n_specials,
                      bpe_result** out);
int bpe_counter_info(const bpe_counter* c, bpe_counter_info_t* out);
/* forget every word; the device memory is kept for the next inputs */
void bpe_counter_clear(bpe_counter* c);
void bpe_counter_free(bpe_counter* c);

/* Hands back the device memory the trainer keeps between calls so that a repeated train_bpe
 * does not pay for fresh allocations: the corpus buffer (drive.hip), the counter's record pool
 * and aggregation bins (count.hip; about 2 x 2 bytes per corpus byte), for `device` (< 0: every
 * device).  The reference keeps nothing after train_bpe returns (train.py:231) and its caller
 * trains an LM on the same GPU next (train.py:230-232), so the Python train_bpe calls this after
 * every call unless keep_device_buffers=True.  Buffers held by a call in flight are not touched,
 * and the cached copy streams (no HBM to speak of) stay for the process, so a transfer of
 * another thread is never cut off.  Tokenizer buffers: bpe_tok_release_buffers.  *freed_bytes (may be
 * NULL): device bytes handed back. */
int bpe_release_device_memory(int device, size_t* freed_bytes);

/* Enable per-launch event timing of the hot kernels (bench / profiling); default off. */
void bpe_set_timing(int enable);

/* ---------------------------------------------------------------- tokenizer */
/* Tokenizer(vocab, merges, special_tokens).  vocab blob: u32 count, then per entry
 * (i64 id, u32 len, bytes) in the caller's dict order (the reverse map keeps the LAST id of a
 * duplicated byte string, tokenizer.py:19).  merges blob: u32 count + merge records.
 * specials: NULL/0 for none.  Missing specials are appended with ids len(vocab), ...
 * (tokenizer.py:35-38); their ids are reported by bpe_tok_special_id.  Vocab ids must lie in
 * [0, 2^32), sparse or dense: the ids come out as uint32.  One outside: BPE_E_ARG. */
int bpe_tok_create(const uint8_t* vocab_blob, size_t vocab_n, const uint8_t* merges_blob,
                   size_t merges_n, const char* const* specials, int n_specials,
                   bpe_tokenizer** out);
int64_t bpe_tok_special_id(const bpe_tokenizer* tok, int i);
/* encode(text): UTF-8 bytes in host memory -> ids.  cap >= n always suffices.
 * Limits of one call (BPE_E_LIMIT): a pre-token under 8 MiB; at most 2^28 word-table slots,
 * i.e. about 134 M distinct pre-tokens at the table's half load (an 11.9 GB OWT-like text has
 * 7.5 M).  A text past that is encoded in pieces cut at safe points (bpe_tok_encode_gpus cuts
 * them that way on one device too), whose concatenated ids are the whole text's. */
int bpe_tok_encode(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, uint32_t* ids_out,
                   size_t cap, size_t* n_out);
/* same, device-resident text and output (d_out holds >= n ids) */
int bpe_tok_encode_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, uint32_t* d_out,
                          size_t* n_out, void* hip_stream);
/* Chunked encode: the ids of encode(text[starts[i] : starts[i+1]]) for every piece, concatenated
 * (starts sorted byte offsets; the last piece runs to n).  A piece boundary ends every
 * pre-token and no special token may straddle it -- exactly separate encode() calls, as the
 * reference's encode_iterable (tokenizer.py:140-150: 2 MiB-character batches) and dataset
 * encoder (encode.py:31-36: 1 M-character reads) make them. */
int bpe_tok_encode_chunks(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* starts,
                          size_t n_starts, uint32_t* ids_out, size_t cap, size_t* n_out);
int bpe_tok_encode_chunks_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* starts,
                                 size_t n_starts, uint32_t* d_out, size_t* n_out, void* hip_stream);
/* Batch encode: encode(doc) for every doc = text[doc_starts[i] : doc_starts[i+1]) (the last runs to
 * n), the ids concatenated; id_offsets gets n_docs + 1 entries: doc i's ids are
 * ids[id_offsets[i] : id_offsets[i+1]).  doc_starts[0] == 0, non-decreasing, <= n, else BPE_E_ARG
 * (equal starts: an empty document).  Exactly separate encode() calls, as the chunked encode
 * above; the offsets are exact where summing the ids' byte lengths is not (several byte strings
 * may share an id, a pre-token equal to a special has no id).  cap >= n always suffices. */
int bpe_tok_encode_batch(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts,
                         size_t n_docs, uint32_t* ids_out, size_t cap, size_t* n_out, uint64_t* id_offsets_out);
/* same, device-resident text, ids (d_out holds >= n) and offsets (n_docs + 1); doc_starts in host memory */
int bpe_tok_encode_batch_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                size_t n_docs, uint32_t* d_out, size_t* n_out, uint64_t* d_id_offsets,
                                void* hip_stream);
/* Encode with offsets: the batch encode above, and for every id the half-open span (start, end) of
 * the text it came from, relative to the start of its own document: spans[2 i], spans[2 i + 1]
 * for id i.  unit 0: bytes -- text[start:end) are the bytes of the merge piece that produced the
 * id (a special token: its own bytes, whether or not the vocab had it).  A pre-token equal to a
 * special yields no id, so the next span starts past it; otherwise the spans of a document tile
 * it, in order and without overlap.  unit 1: characters -- with C(p) = the bytes of text[0:p)
 * that are not continuation bytes (b & 0xC0 != 0x80), start = C(start) - (1 if text[start] is a
 * continuation byte), end = C(end): a byte-level token that begins or ends inside a character
 * covers that character.  Any other unit: BPE_E_ARG.  The text is valid UTF-8 (every document on
 * its own).  Limits: a document of 2^32 bytes or more is BPE_E_LIMIT; a vocab in which one id
 * names byte strings of different lengths has no per-id length, and both calls refuse it with
 * BPE_E_ARG (decided at bpe_tok_create; the other encode calls are unaffected).  cap >= n and
 * spans_cap >= n (in spans, 8 bytes each) always suffice. */
int bpe_tok_encode_spans(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts,
                         size_t n_docs, int unit, uint32_t* ids_out, size_t cap, size_t* n_out,
                         uint64_t* id_offsets_out, uint32_t* spans_out, size_t spans_cap);
/* same, device-resident text, ids (d_ids holds >= n), offsets (n_docs + 1) and spans (d_spans holds
 * >= n spans of two uint32 and is 8-byte aligned); doc_starts in host memory.  One call at a time
 * per tokenizer, on the current device, as the batch calls; the scratch it adds is released by
 * bpe_tok_release_buffers. */
int bpe_tok_encode_spans_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                size_t n_docs, int unit, uint32_t* d_ids, size_t* n_out, uint64_t* d_id_offsets,
                                uint32_t* d_spans, void* hip_stream);
/* Encode with BPE-dropout (Provilkov et al., 2020): the batch encode above, except that while a
 * pre-token is merged every candidate merge is skipped with probability thr / 2^24.  Segmentation
 * on specials, pre-tokenization, the dropping of a pre-token equal to a special and the id lookup
 * (BPE_E_KEY) are those of bpe_tok_encode; a special yields its one id and draws nothing.  The draws
 * are counter-based (mix64: z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 * z *= 0x94D049BB133111EB, z ^ z >> 31, all mod 2^64):
 *     wk      = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ doc_key) ^ off)
 *     dropped = (mix64(wk ^ (round << 32 | pos)) >> 40) < thr
 * off: the byte offset of the pre-token's first byte in its document; round 0, 1, ...: the merge
 * rounds of that pre-token; pos: the byte offset, inside the pre-token, of the pair's left token.
 * A round merges, left to right, every occurrence that is not dropped of the ranked pair of lowest
 * rank among the positions not dropped; when there is none the pre-token is done, also when
 * ranked pairs remain.  Document i of the call draws with doc_key = doc_base + i, so a document's
 * ids depend on (seed, doc_key, text) alone: not on the batch it is in, nor on the device's order
 * of work or the pointers' alignment.  thr 0 is bpe_tok_encode_batch exactly; thr 2^24 gives every
 * byte its own id; thr > 2^24 or doc_base + n_docs past 2^64: BPE_E_ARG.  (thr = round(p * 2^24)
 * is computed by the caller: no float crosses the ABI.)  Limits: a document of 2^32 bytes or more,
 * a pre-token of 8 MiB or more: BPE_E_LIMIT.  cap >= n always suffices. */
int bpe_tok_encode_dropout(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts,
                           size_t n_docs, uint32_t thr, uint64_t seed, uint64_t doc_base, uint32_t* ids_out,
                           size_t cap, size_t* n_out, uint64_t* id_offsets_out);
/* same, device-resident text, ids (d_ids holds >= n; the call also uses it as scratch) and offsets
 * (n_docs + 1); doc_starts in host memory.  One call at a time per tokenizer, on the current device,
 * as the batch calls; the scratch it adds is released by bpe_tok_release_buffers. */
int bpe_tok_encode_dropout_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                  size_t n_docs, uint32_t thr, uint64_t seed, uint64_t doc_base, uint32_t* d_ids,
                                  size_t* n_out, uint64_t* d_id_offsets, void* hip_stream);
/* CSR ids (as the batch encode returns them) -> a dense [n_rows, row_len] matrix of int32
 * (elem_bytes 4) or int64 (8) in d_out, and d_lengths[i] = min(L_i, row_len).  A row longer than
 * row_len keeps its first ids (flags & 1: its last); a shorter one is filled with pad on the
 * right (flags & 2: on the left).  All pointers device memory; returns once the matrix is written.
 * With elem_bytes 4 a kept id that does not fit int32 (2^31 or more) is an error, BPE_E_LIMIT with
 * the smallest such id in the message, instead of a negative entry (the matrix is then not to be
 * used); an id that the truncation drops is not looked at.  elem_bytes 8 holds every id. */
int bpe_ids_pack_rows_device(const uint32_t* d_ids, const uint64_t* d_offsets, size_t n_rows, size_t row_len,
                             int64_t pad, int flags, int elem_bytes, void* d_out, int32_t* d_lengths,
                             void* hip_stream);
/* The reference's dataset encoder (encode.py:18-38) on one file: the file is read by the library's
 * pinned multi-threaded reader into HBM, decoded as open(path, "r", encoding="utf-8") reads it
 * (strict UTF-8, universal newlines), cut into chars_per_piece-character pieces (f.read(1024*1024)),
 * each piece encoded on its own, and the ids written as np.uint16 (encode.py:37; an id past
 * 65535 fails with BPE_E_LIMIT instead of wrapping) into ids_out (host memory, cap ids; the
 * file's byte count always suffices).  The device buffers are kept by the tokenizer across
 * calls (about 3 bytes of HBM per file byte: the text and its uint16 ids, on top of the
 * encoder's per-call arrays) until bpe_tok_release_buffers or bpe_tok_free.  The stages overlap:
 * the file streams in by 1 GiB slabs while the pieces already read
 * are validated, encoded and copied out (a text with a carriage return is redone in one pass
 * once read).  phase_ms (NULL or 4 doubles): busy milliseconds of the reader, of validation +
 * piece starts, of the encodes and of the copy to host. */
int bpe_tok_encode_file_u16(bpe_tokenizer* tok, const char* path, size_t chars_per_piece, uint16_t* ids_out,
                            size_t cap, size_t* n_out, double* phase_ms);
/* The dataset encoder over many files of any size: every file is encoded exactly as
 * bpe_tok_encode_file_u16 encodes it alone (text-mode read, pieces of chars_per_piece characters of
 * the translated text counted from the start of that file, each piece on its own), the files' ids
 * are concatenated in the order of paths and written to out_path as raw little-endian ids of
 * id_bytes each (what np.memmap(path, dtype) reads).
 *
 * Read grid and carry: the raw bytes of each file are read in consecutive ranges of exactly
 * window_bytes (0: 1 GiB, a choice and not a measured optimum; else at least 65536), the last
 * range shorter.  What a range cannot finish waits for the next one: bpe_window_holdback bytes of
 * its end (an incomplete UTF-8 character, a final \r that may be half of \r\n), and, of the
 * translated text, the bytes after the last piece start found (a window edge is not a piece edge).
 * A piece longer than a window grows the text buffer for that piece only (stats->n_grows).
 *
 * Memory.  Device: two raw read buffers of window_bytes + 32; one translated-text buffer of the
 * carry (less than one piece) + window_bytes + 64; two id buffers of id_bytes per byte of that
 * text buffer; while a window that holds a \r is translated, three more arrays of its size; the
 * separator positions of one region (8 bytes per match, at least 64 KiB); the n_counts table; on
 * top of the encoder's per-call arrays for one region.  stats->device_bytes is what this call's
 * buffers held at most.  The buffers stay with the tokenizer until bpe_tok_release_buffers.  Host:
 * the ids of one region.  Nothing grows with a file's or the corpus' size.  Input that is not a
 * regular file (a FIFO) is read to its end into host memory first.
 *
 * opts->has_separator: the positions p of the whole output stream with ids[p] == separator_id go
 * to index_path, ascending, as raw little-endian uint64 (index_path is required then, and must be
 * NULL otherwise).  id_counts (NULL, or n_counts entries in host memory): set to the occurrences of
 * every id, accumulated on the device in 64 bits; an emitted id at or above n_counts is BPE_E_ARG.
 * file_id_offsets (NULL or n_paths + 1 entries): file i's ids are [offsets[i], offsets[i + 1]).
 *
 * Errors: a file that cannot be opened or read is BPE_E_IO with errno; ill-formed UTF-8 is
 * BPE_E_UTF8 whose message gives the byte's position in that raw file and the file's name; an id
 * that does not fit id_bytes == 2 is BPE_E_LIMIT, never a wrapped id.  Both outputs are written
 * under a temporary name beside their path and renamed when the whole call has succeeded: after
 * an error out_path and index_path are as they were, absent or the old file untouched.
 * The stages overlap: a reader thread fills the next raw buffer and a writer thread copies out and
 * pwrites the previous region's ids while the current one is decoded and encoded.  Runs on the
 * current device; one call at a time per tokenizer. */
typedef struct bpe_dataset_opts {
    size_t chars_per_piece;   /* > 0 */
    size_t window_bytes;      /* 0: the 1 GiB default */
    int id_bytes;             /* 2 (uint16) or 4 (uint32) */
    int has_separator;
    uint64_t separator_id;
    const char* index_path;
} bpe_dataset_opts;
typedef struct bpe_dataset_stats {
    uint64_t n_ids, n_bytes, n_pieces, n_windows, max_window_bytes, n_separators, device_bytes, n_grows;
    /* busy milliseconds (they overlap): the reader; validation, newlines and piece starts; the
     * encodes; the copy-out and pwrite; the histogram and the separator search */
    double read_ms, decode_ms, encode_ms, write_ms, stats_ms;
} bpe_dataset_stats;
int bpe_tok_encode_files(bpe_tokenizer* tok, const char* const* paths, size_t n_paths, const char* out_path,
                         const bpe_dataset_opts* opts, uint64_t* file_id_offsets, uint64_t* id_counts,
                         size_t n_counts, bpe_dataset_stats* stats);
/* How many of the last n (at most the last 4 are looked at) raw bytes of a read range must wait
 * for the next range: the longest suffix that is a proper prefix of a well-formed UTF-8 sequence,
 * else 1 for a final \r (it may be the first half of \r\n), else 0; always 0 with at_eof.  Host
 * only; the dataset encoder's carry uses this very function. */
size_t bpe_window_holdback(const uint8_t* tail, size_t n, int at_eof);
/* d_counts[id] += occurrences of id in d_ids[0, n), 64-bit (the table accumulates over calls).
 * d_ids: ids of elem_bytes 2, 4 or 8 (unsigned; an 8-byte id must lie in [0, 2^32)) in device
 * memory, aligned to elem_bytes only; d_counts: n_counts <= 2^32 uint64 in device memory.  An id
 * at or above n_counts is BPE_E_ARG with the smallest such id in the message, and the table is
 * then not to be used.  Frequent ids below 8192 are counted in LDS per workgroup and flushed with
 * 64-bit adds.  Returns once the table is updated. */
int bpe_ids_histogram_device(const void* d_ids, size_t n, int elem_bytes, uint64_t* d_counts, size_t n_counts,
                             void* hip_stream);
/* base + i for every i with d_ids[i] == value, ascending, into d_pos_out (device, cap entries);
 * *n_out = how many there are, which may exceed cap (then only the first cap were written: call
 * again with room for all).  d_ids as above.  Returns once the positions are written. */
int bpe_ids_find_device(const void* d_ids, size_t n, int elem_bytes, uint64_t value, uint64_t base,
                        uint64_t* d_pos_out, size_t cap, size_t* n_out, void* hip_stream);
/* The batch loader (the reference's load_batch, models/util.py:37-57): windows of an id stream ->
 * the dense matrices of a training step, in one launch.  For every row r < n_rows and t < row_len
 *     inputs[r, t]  = ids[src[r] + t]
 *     targets[r, t] = ids[src[r] + t + 1]          (d_targets NULL: not written)
 * int32 (out_elem_bytes 4) or int64 (8), row-major [n_rows, row_len].  Each row's row_len + 1 ids are
 * read once, as 16-byte vectors on the 16-byte grid, and both matrices are written from them with
 * 16-byte stores wherever the output's alignment allows.  All pointers are device memory.
 *
 * d_ids: n ids of elem_bytes 2 or 4 (unsigned), aligned to elem_bytes only.  d_src: n_rows int64
 * offsets into d_ids.  d_pos: NULL, or n_rows int64: the rows' positions in the whole stream when
 * d_ids is not that stream (the staged path below gathers the rows first); NULL: pos = src.
 *
 * Document-aware outputs, from the sorted separator positions d_sep_pos[n_sep] (what encode_files
 * writes to index_path; a separator ends a document and belongs to it), with g = pos[r] + t:
 *     positions[r, t] = g - (the largest separator position < g, or -1) - 1       int64
 *     doc_ids[r, t]   = the number of separator positions in [pos[r], g)           int32
 * Either may be NULL.  Both are computed from the index alone (n_sep == 0 is valid: the position is
 * then g itself), not from the ids.
 * flags & BPE_BATCH_IGNORE: targets[r, t] = ignore_index where inputs[r, t] == separator_id.
 *
 * Checks, on the device.  No load falls outside d_ids[0, n): a row with src[r] < 0 or src[r] > n -
 * row_len - 1 (n - row_len without targets) is neither read nor written.  With out_elem_bytes 4 an id
 * of 2^31 or more that is written is reported (the matrices are then not to be used); ids outside
 * every row are not looked at.  Both reports go through the 8-byte word d_status (NULL: nothing is
 * reported), which the call sets to ~0 first.  flags & BPE_BATCH_CHECK (d_status required): the
 * word is copied back, the stream is synchronised, and the call returns BPE_E_ARG with "row <r>
 * starts outside [0, <last valid>]" for the smallest such row, else BPE_E_LIMIT with the smallest
 * such id in the message, as bpe_ids_pack_rows_device.  Without the bit the call only enqueues on
 * hip_stream and returns; the word then holds ~0, the smallest bad row, or 2^62 | the smallest id.
 * row_len >= 1; n_rows == 0 is valid.  Runs on the current device. */
#define BPE_BATCH_CHECK 1
#define BPE_BATCH_IGNORE 2
typedef struct bpe_batch_args {
    size_t n_rows, row_len;
    int out_elem_bytes;          /* 4 or 8: inputs and targets */
    int flags;
    void* d_inputs;
    void* d_targets;             /* NULL: none */
    int64_t* d_positions;        /* NULL: none */
    int32_t* d_doc_ids;          /* NULL: none */
    const uint64_t* d_sep_pos;
    size_t n_sep;
    uint64_t separator_id;       /* BPE_BATCH_IGNORE */
    int64_t ignore_index;
    uint64_t* d_status;
} bpe_batch_args;
int bpe_ids_batch_rows_device(const void* d_ids, size_t n, int elem_bytes, const int64_t* d_src,
                              const int64_t* d_pos, const bpe_batch_args* args, void* hip_stream);
/* The same for a stream in host memory (an array, an np.memmap of a file that is not to be held in
 * HBM): ids[0, n) and starts[n_rows] are host memory, the outputs in args device memory.  At most 8
 * host threads (one per 512 KiB of rows) copy the rows' row_len + 1 ids each into a pinned buffer
 * behind the rows' offsets, one hipMemcpyAsync moves that buffer to a device buffer of the handle,
 * and the kernel above runs on it with pos = starts.  starts are checked on the host (BPE_E_ARG,
 * the message as above) before anything is enqueued.  The handle owns two pinned and two device
 * buffers with an event each and alternates between them: a call waits only for the copy and the
 * kernel of the call before the previous one, so two calls in a row are issued without a
 * synchronisation.  Buffers grow as needed and stay until bpe_batch_stage_free.  A handle belongs
 * to the device current at its creation; one caller at a time. */
typedef struct bpe_batch_stage bpe_batch_stage;
int bpe_batch_stage_create(bpe_batch_stage** out);
int bpe_batch_stage_rows(bpe_batch_stage* stage, const void* ids, size_t n, int elem_bytes, const int64_t* starts,
                         const bpe_batch_args* args, void* hip_stream);
void bpe_batch_stage_free(bpe_batch_stage* stage);
/* encode(text) on n_gpus devices of this process (<= 0: every visible one; SURVEY.md 8b's n_gpus):
 * the text is cut at safe split points that no special token spans, each device encodes its
 * piece, the ids are concatenated -- identical to bpe_tok_encode (tokenizer.py:111-138). */
int bpe_tok_encode_gpus(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, uint32_t* ids_out, size_t cap,
                        size_t* n_out, int n_gpus);
/* Frees the device buffers the tokenizer keeps across calls (the encoder's record and scratch
 * arrays, the bulk encoder's text and uint16 ids, the other devices' copies); the next call
 * allocates them again.  The tables of the tokenizer itself stay. */
int bpe_tok_release_buffers(bpe_tokenizer* tok);
void bpe_tok_free(bpe_tokenizer* tok);

/* ---------------------------------------------------------------- decode */
/* Tokenizer.decode (tokenizer.py:155-157): b"".join(vocab[i] for i in ids) on the device; the
 * caller applies .decode("utf-8", errors="replace").  vocab blob: u32 count, then (i64 id,
 * u32 len, bytes) per entry -- the int-keyed entries of Tokenizer.vocab.  An id without an
 * entry fails with BPE_E_KEY (message: the id), as vocab[i] raises KeyError.  Vocab ids must lie
 * in [0, 2^28): the decoder keeps a dense table up to the largest id (the encoder takes ids up to
 * 2^32 - 1).  One outside: BPE_E_LIMIT from bpe_dec_create. */
typedef struct bpe_decoder bpe_decoder;
int bpe_dec_create(const uint8_t* vocab_blob, size_t vocab_n, bpe_decoder** out);
/* host ids -> host bytes; *n_out = byte count (also set when cap is too small: BPE_E_ARG) */
int bpe_dec_decode(bpe_decoder* dec, const uint32_t* ids, size_t n, uint8_t* out, size_t cap, size_t* n_out);
/* device ids -> device bytes */
int bpe_dec_decode_device(bpe_decoder* dec, const uint32_t* d_ids, size_t n, uint8_t* d_out, size_t cap,
                          size_t* n_out, void* hip_stream);
/* Batch decode: decode(ids[id_offsets[i] : id_offsets[i+1]]) for every row i, the rows' bytes
 * concatenated, in one launch sequence without a size-query pass.
 * id_offsets: n_rows + 1 entries, id_offsets[0] == 0, non-decreasing, last == n, else BPE_E_ARG
 * (equal neighbours: an empty row).  *bytes_out: malloc'ed, release with bpe_blob_free (never NULL
 * on success, also for 0 bytes).  byte_offsets_out: n_rows + 1 entries: row i's bytes are
 * bytes[byte_offsets[i] : byte_offsets[i+1]).  token_offsets_out: NULL, or n + 1 entries: token
 * j's bytes are bytes[token_offsets[j] : token_offsets[j+1]).  An id without a vocab entry:
 * BPE_E_KEY, message = the id, the first such id in flat order.  n == 0 and n_rows == 0 are valid. */
int bpe_dec_decode_batch(bpe_decoder* dec, const uint32_t* ids, size_t n, const uint64_t* id_offsets,
                         size_t n_rows, uint8_t** bytes_out, size_t* n_bytes,
                         uint64_t* byte_offsets_out, uint64_t* token_offsets_out);
/* same, everything in device memory (d_id_offsets too: it is checked on the device); cap too small:
 * BPE_E_ARG with *n_out = bytes needed, as bpe_dec_decode_device (d_byte_offsets and d_token_offsets
 * are written then as well).  d_token_offsets may be NULL.  hip_stream NULL: the decoder's own
 * stream, as in bpe_dec_decode_device.  Returns once d_out is written.  The decoder keeps the
 * batch calls' device arrays between calls while they take at most 64 MiB; one call at a time
 * uses them (the calls of several threads on one decoder take turns). */
int bpe_dec_decode_batch_device(bpe_decoder* dec, const uint32_t* d_ids, size_t n,
                                const uint64_t* d_id_offsets, size_t n_rows, uint8_t* d_out, size_t cap,
                                size_t* n_out, uint64_t* d_byte_offsets, uint64_t* d_token_offsets,
                                void* hip_stream);
/* A dense [n_rows, row_len] matrix of ids in device memory (elem_bytes 4: int32, 8: int64), as
 * bpe_ids_pack_rows_device writes it or a generation loop fills it, -> host bytes and row offsets
 * as bpe_dec_decode_batch returns them; the ids never visit the host.  The kept span of row i:
 * with d_lengths (int32, n_rows entries) its first d_lengths[i] entries (flags & 2: its last, a
 * left-padded row), without (NULL) all row_len; with stop_id >= 0 the span ends before the first
 * entry equal to stop_id (flags & 1: after it).  A length outside [0, row_len]: BPE_E_ARG.
 * Entries outside the kept span are never inspected (any pad value is legal there); a kept entry
 * outside [0, 2^32) or without a vocab entry: BPE_E_KEY, message = the entry in decimal, the first
 * such entry in row-major order.  n_rows == 0 and row_len == 0 are valid. */
int bpe_dec_decode_rows_device(bpe_decoder* dec, const void* d_rows, int elem_bytes, size_t n_rows,
                               size_t row_len, const int32_t* d_lengths, int64_t stop_id, int flags,
                               uint8_t** bytes_out, size_t* n_bytes, uint64_t* byte_offsets_out,
                               void* hip_stream);
void bpe_dec_free(bpe_decoder* dec);

/* ---------------------------------------------------------------- bulk encode plumbing */
/* The raw bytes of a regular file -> device memory d_dst (cap bytes): pread by a pool of host
 * threads into pinned staging buffers, each DMA'd to HBM while the next is read (the file read
 * of encode.py:31-33 / tokenizer.py:111, without a pageable host copy).  d_dst == NULL: size
 * query (*n_out = file size).  BPE_E_IO (errno) on a missing file, a directory, or a file that
 * is not regular (the caller reads a pipe itself); BPE_E_ARG if cap is too small. */
int bpe_read_file_device(const char* path, uint8_t* d_dst, size_t cap, size_t* n_out);
/* n bytes of device memory -> pageable host memory h_dst (e.g. the np.uint16 array encode.py
 * saves), through pinned staging buffers, several copier threads; waits for the device first. */
int bpe_copy_to_host(const void* d_src, size_t n, void* h_dst);
/* open(path, "r", encoding="utf-8").read() on device bytes: strict UTF-8 (BPE_E_UTF8) and
 * universal newlines.  d_out holds n bytes (may be d_in); *n_out = resulting length. */
int bpe_text_prepare_device(const uint8_t* d_in, size_t n, uint8_t* d_out, size_t* n_out, void* hip_stream);
/* Byte offsets of characters 0, K, 2K, ... of valid UTF-8 (K = chars_per_chunk): the pieces
 * successive f.read(K) calls return (encode.py:31-33).  starts == NULL: count only. */
int bpe_utf8_chunk_starts_device(const uint8_t* d_text, size_t n, size_t chars_per_chunk, uint64_t* starts,
                                 size_t cap, size_t* n_starts, void* hip_stream);
/* np.array(token_ids, dtype=np.uint16) (encode.py:37), on the device; BPE_E_LIMIT if an id
 * does not fit (the reference would silently wrap it). */
int bpe_ids_to_u16_device(const uint32_t* d_ids, size_t n, uint16_t* d_out, void* hip_stream);

/* ---------------------------------------------------------------- ill-formed UTF-8 */
/* Every entry point above that reads text decodes it strictly (BPE_E_UTF8).  The calls below add
 * CPython's errors="replace" (mode 1) and errors="ignore" (mode 2): each maximal subpart of an
 * ill-formed subsequence becomes one U+FFFD (EF BF BD) or is dropped, exactly
 * bytes.decode("utf-8", errors).  Mode 0 is strict and runs exactly the code of the call it
 * extends.  A clean input pays nothing: the repair runs only after the strict validation failed. */
#define BPE_UTF8_STRICT 0
#define BPE_UTF8_REPLACE 1
#define BPE_UTF8_IGNORE 2
typedef struct bpe_utf8_stats {
    uint64_t n_units;   /* spans replaced or dropped */
    uint64_t n_bytes;   /* the input bytes they covered */
    uint64_t first;     /* where the first span starts (what strict mode reports), ~0: none */
} bpe_utf8_stats;
/* d_out[0, *n_out) = bytes(d_in[0, n)).decode("utf-8", errors).encode("utf-8") for mode 1 or 2,
 * all in device memory on the current device; d_in is not modified and must not overlap d_out.
 * d_out == NULL: size query (*n_out and *stats are set, nothing is written).  cap < *n_out:
 * BPE_E_ARG with *n_out set.  Replace grows a text up to 3x; the offsets are 64-bit.  stats may be
 * NULL.  Returns once d_out is written. */
int bpe_utf8_repair_device(const uint8_t* d_in, size_t n, int mode, uint8_t* d_out, size_t cap, size_t* n_out,
                           bpe_utf8_stats* stats, void* hip_stream);
/* the repair kernel's vector width (bytes a thread classifies) and tile (bytes a workgroup
 * repairs per step): where its code paths meet, for tests */
int bpe_utf8_repair_geometry(size_t* unit_bytes, size_t* tile_bytes);
/* bpe_text_prepare_device with an errors mode: the repair, then universal newlines.  d_out ==
 * NULL: *n_out = the bytes d_out must hold (the repaired length; the translated text is no
 * longer).  d_out may be d_in when it holds that many bytes. */
int bpe_text_prepare_device_ex(const uint8_t* d_in, size_t n, int mode, uint8_t* d_out, size_t cap, size_t* n_out,
                               bpe_utf8_stats* stats, void* hip_stream);
/* The errors mode of a counter's later bpe_counter_add_file / _add_buffer / _add_device calls
 * (0 at creation).  In mode 1 or 2 a window whose validation fails is repaired where it lies in
 * HBM and counted again; windows end at ASCII bytes, so the result is the whole file's. */
int bpe_counter_set_errors(bpe_counter* c, int mode);
/* what the last such call repaired; first is a position in that input */
int bpe_counter_utf8_report(const bpe_counter* c, bpe_utf8_stats* out);
/* The errors mode of a tokenizer's later bpe_tok_encode_files calls (0 at creation): a raw range
 * that fails validation is repaired before the newline translation; pieces count characters of
 * the repaired text (U+FFFD is one). */
int bpe_tok_set_errors(bpe_tokenizer* tok, int mode);
/* what the last bpe_tok_encode_files call repaired: the totals (first: a position in the raw
 * file *first_file, an index into paths), and per file the spans (file_units: NULL or n_files
 * entries; files beyond the last call's count get 0) */
int bpe_tok_utf8_report(const bpe_tokenizer* tok, bpe_utf8_stats* total, uint64_t* first_file,
                        uint64_t* file_units, size_t n_files);

/* ---------------------------------------------------------------- helpers */
/* Largest p <= pos such that splitting the text at p does not change its pre-tokenization
 * (a U+0020 between two ASCII non-space bytes), or 0. Used to shard a corpus into slabs. */
size_t bpe_safe_split(const uint8_t* data, size_t n, size_t pos);
/* Deterministic synthetic corpus (bench/tests): bytes [first_block*4096, first_block*4096 + n)
 * of corpus (seed, flavour) into device memory; flavour 0 = OWT-like, 1 = TinyStories-like.
 * Every 4096-byte block boundary is a safe split point, so slabs of whole blocks shard it. */
int bpe_synth_corpus_device(uint8_t* d_out, size_t n, uint64_t seed, int flavour,
                            uint64_t first_block, void* hip_stream);
/* The same bytes written by the host (n_threads CPU threads), for the oracle side of the
 * large parity checks; needs no device. */
int bpe_synth_corpus_host(uint8_t* out, size_t n, uint64_t seed, int flavour,
                          uint64_t first_block, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* BPE355_H */
