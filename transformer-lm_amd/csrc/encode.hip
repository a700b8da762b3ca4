// Tokenizer.encode on the device -- reference models/tokenizer/tokenizer.py:
//   12-38   construction: vocab_inv (last id wins), specials deduped + longest first,
//           missing specials appended with ids len(vocab), len(vocab)+1, ...
//   63-66   segment: re.split on the specials alternation (leftmost match, longest first)
//   68-90   pretokenize each non-special segment on its own with the GPT-2 pattern; drop
//           matches equal to a special; special segments stay whole
//   92-138  per pretoken: repeatedly merge ALL occurrences of the adjacent pair with the lowest
//           merge rank (ties: leftmost) until no pair is ranked; ids via vocab_inv (KeyError)
//
// Device pipeline (one stream):
//   0. (once per tokenizer) build_dictionary: every vocab entry of 2..16 bytes encoded by
//      k_encode_words into an L2-sized open-addressing table, and the one-byte words' ids.
//   1. k_find_specials marks where a special starts (first-byte bitmap, then compare); the
//      sorted matches become the segment table on the device (k_sp_*), or on the host when
//      matches overlap.
//   2. k_enc_scan4: persistent workgroups stage 16 KiB chunks in LDS, evaluate the token-start
//      predicate per 64-byte block, and write one u32 record per pre-token, each chunk's records
//      one dense run: a direct id (one-byte words, one-id dictionary words, via an LDS word
//      cache), a special, a dictionary entry, or the slot of a word-table entry (the long tail).
//   3. k_collect + k_encode_words: the word table's words get their rank-ordered merges once
//      (after step 4's resolve has inserted them).
//   4. k_enc_resolve_c: the scan's pending words (LDS-cache misses) -> a dictionary word's ids'
//      info, or a word-table slot, in a kernel with registers to spare; k_enc_finalize: the
//      table words' slots -> their ids' info.
//   5. k_enc_emit<count>, an exclusive scan of the chunks' id counts, k_enc_emit<write>: per
//      chunk, ids assembled in LDS and stored with coalesced writes.
//   5'. (encode_batch) the scan also notes, per document start, the record of the token that
//      starts there; k_enc_cut_offsets turns those into id offsets with one more pass over the
//      records, k_enc_doc_offsets hands every document its own.
//   6. k_pack_rows: ids and offsets -> padded rows.
//   (encode with dropout) steps 1 and 2 only, the scan in its kCuts, kPos instantiation; every
//      occurrence then merges on its own in dropout.hip (dropout_emit), which reads the records.

#include <algorithm>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "drive.h"
#include "internal.h"
#include "prims.h"
#include "pretok.h"
#include "stage.h"
#include "stage2.h"
#include "utf8fix.h"

namespace bpe {
namespace {

constexpr unsigned long long kOff40 = (1ULL << 40) - 1;

struct Seg {                 // a piece of the text: normal (special = -1) or one special token
    unsigned long long start, end;
    int special;
    int pad;
};

struct EncTables {
    const unsigned long long* pm_key;  // ((a << 32) | b) + 1
    const uint2* pm_val;               // (rank, product)
    unsigned long long pm_mask;
    const int64_t* tok2vid;            // internal token -> vocab id, -1 if absent
    const uint32_t* byte2tok;          // 256 entries
    const uint8_t* sp_bytes;
    const uint32_t* sp_off;
    const uint32_t* sp_len;
    const int64_t* sp_vid;
    int n_sp;
};

__device__ __forceinline__ bool bytes_eq(const uint8_t* x, const uint8_t* y, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (x[i] != y[i]) return false;
    return true;
}

// bytes [gp, gp + len) of s (len <= 16) packed little-endian, with aligned 8-byte loads (three at
// most) when the text runs on past them, else byte by byte
__device__ __forceinline__ void load_word(const uint8_t* __restrict__ s, size_t n, size_t gp, size_t len,
                                          uint64_t& lo, uint64_t& hi) {
    if (gp + 24 > n) {
        pack_word(s, gp, len, lo, hi);
        return;
    }
    const uintptr_t addr = reinterpret_cast<uintptr_t>(s + gp);
    const uint64_t* a = reinterpret_cast<const uint64_t*>(addr & ~(uintptr_t)7);
    const unsigned sh = (unsigned)(addr & 7) * 8;
    const uint64_t q0 = a[0], q1 = a[1];
    const uint64_t q2 = (addr & 7) + len > 16 ? a[2] : 0;
    lo = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
    hi = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
    if (len < 8) {
        lo &= (1ULL << (8 * len)) - 1;
        hi = 0;
    } else if (len < 16) {
        hi &= (1ULL << (8 * (len - 8))) - 1;
    }
}

// ------------------------------------------------------------------ 1. special candidates
// Matches are appended as position << 16 | special index (sorted on the device afterwards).
constexpr int kSpShift = 16;

constexpr int kSpLds = 64;   // specials whose first 16 bytes k_find_specials keeps in LDS
constexpr unsigned kSpBuf = 2048;   // matches a workgroup of k_find_specials stages in LDS

__global__ void __launch_bounds__(256) k_find_specials(const uint8_t* __restrict__ s, size_t n, EncTables E,
                                                       const unsigned* __restrict__ first_mask,
                                                       unsigned long long* __restrict__ key_out,
                                                       unsigned* __restrict__ n_out, unsigned long long cap) {
    // Every special matching at i is recorded (sorted longest first, the host takes the first
    // that fits): when the longest one straddles a piece cut, re.split on that piece still
    // matches a shorter special that is its prefix (tokenizer.py:63-66).
    // A thread takes 16-byte units (aligned loads, two in flight; the text is streamed once),
    // marks the bytes that may start a special (first-byte bitmap) and compares only those: the
    // 16 bytes at a candidate against the specials' first 16 (LDS), the rest byte by byte.
    // Grid-stride, the trip count uniform over the workgroup (the candidate loop's __any).
    __shared__ unsigned s_fm[8];
    __shared__ uint64_t s_lo[kSpLds], s_hi[kSpLds];
    __shared__ uint32_t s_len[kSpLds];
    // the workgroup's matches, flushed with one global reservation at the end (a device-scope
    // atomic per wave that found one: millions of them on one word would serialise at ~88/us)
    __shared__ unsigned long long s_keys[kSpBuf];
    __shared__ unsigned s_nk, s_base;
    if (threadIdx.x == 0) s_nk = 0;
    if (threadIdx.x < 8) s_fm[threadIdx.x] = first_mask[threadIdx.x];
    const int nsl = E.n_sp < kSpLds ? E.n_sp : kSpLds;
    if ((int)threadIdx.x < nsl) {
        const uint32_t l = E.sp_len[threadIdx.x];
        uint64_t lo = 0, hi = 0;
        const uint8_t* p = E.sp_bytes + E.sp_off[threadIdx.x];
        for (uint32_t j = 0; j < l && j < 16; ++j) {
            if (j < 8) lo |= (uint64_t)p[j] << (8 * j);
            else hi |= (uint64_t)p[j] << (8 * (j - 8));
        }
        s_lo[threadIdx.x] = lo;
        s_hi[threadIdx.x] = hi;
        s_len[threadIdx.x] = l;
    }
    __syncthreads();
    const uint8_t* const a0 = s - (reinterpret_cast<uintptr_t>(s) & 15);   // (global address space kept)
    const size_t lead = (size_t)(s - a0);
    const size_t nv = (n + lead + 15) / 16;   // 16-byte units covering [s, s + n)
    const size_t S = (size_t)gridDim.x * blockDim.x;
    auto unit = [&](size_t v, uint32_t (&w)[4]) -> unsigned {   // candidate bits of unit v
        unsigned cm = 0;
        const long long p0 = (long long)(16 * v) - (long long)lead;   // text position of byte 0
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long long p = p0 + j;
            const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            if (p >= 0 && p < (long long)n && ((s_fm[b >> 5] >> (b & 31)) & 1u)) cm |= 1u << j;
        }
        return cm;
    };
    auto load = [&](size_t v, uint32_t (&w)[4]) {
        w[0] = w[1] = w[2] = w[3] = 0;
        if (v >= nv) return;
        const long long p0 = (long long)(16 * v) - (long long)lead;
        if (p0 >= 0 && p0 + 16 <= (long long)n) {
            const uint4 q = *reinterpret_cast<const uint4*>(a0 + 16 * v);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            for (int j = 0; j < 16; ++j) {
                const long long p = p0 + j;
                if (p >= 0 && p < (long long)n) w[j >> 2] |= (uint32_t)s[p] << (8 * (j & 3));
            }
        }
    };
    auto check = [&](size_t v, unsigned cm) {
        for (int j = 0; j < 16; ++j) {
            const bool cand = (cm >> j) & 1u;
            if (!__any(cand)) continue;
            const size_t i = 16 * v + j - lead;
            uint64_t tl = 0, th = 0;
            if (cand) load_word(s, n, i, n - i < 16 ? n - i : 16, tl, th);
            for (int k = 0; k < E.n_sp; ++k) {
                bool hit = false;
                if (cand) {
                    const uint32_t l = k < kSpLds ? s_len[k] : E.sp_len[k];
                    if (i + l <= n) {
                        if (k < kSpLds) {
                            const uint64_t mlo = l >= 8 ? ~0ULL : (1ULL << (8 * l)) - 1;
                            const uint64_t mhi = l >= 16 ? ~0ULL : (l <= 8 ? 0ULL : (1ULL << (8 * (l - 8))) - 1);
                            hit = ((tl ^ s_lo[k]) & mlo) == 0 && ((th ^ s_hi[k]) & mhi) == 0 &&
                                  (l <= 16 || bytes_eq(s + i + 16, E.sp_bytes + E.sp_off[k] + 16, l - 16));
                        } else {
                            hit = bytes_eq(s + i, E.sp_bytes + E.sp_off[k], l);
                        }
                    }
                }
                if (hit) {
                    const unsigned long long key = ((unsigned long long)i << kSpShift) | (unsigned)k;
                    const unsigned li = atomicAdd(&s_nk, 1u);
                    if (li < kSpBuf) {
                        s_keys[li] = key;
                    } else {   // the buffer is full: straight to the global list
                        const unsigned idx = atomicAdd(n_out, 1u);
                        if (idx < cap) key_out[idx] = key;
                    }
                }
            }
        }
    };
    for (size_t v0 = (size_t)blockIdx.x * blockDim.x; v0 < nv; v0 += 2 * S) {
        const size_t va = v0 + threadIdx.x, vb = va + S;
        uint32_t wa[4], wb[4];
        load(va, wa);
        load(vb, wb);
        const unsigned ca = va < nv ? unit(va, wa) : 0u, cb = vb < nv ? unit(vb, wb) : 0u;
        if (__any(ca != 0)) check(va, ca);
        if (__any(cb != 0)) check(vb, cb);
    }
    __syncthreads();
    const unsigned nk = s_nk < kSpBuf ? s_nk : kSpBuf;
    if (threadIdx.x == 0) s_base = nk ? atomicAdd(n_out, nk) : 0u;
    __syncthreads();
    for (unsigned q = threadIdx.x; q < nk; q += blockDim.x)
        if (s_base + q < cap) key_out[s_base + q] = s_keys[q];
}

// ------------------------------------------------------------------ 1'. segments on the device
// The sorted matches (position << 16 | index) become the segment table without a host pass when
// the matches that no piece cut splits (a cut strictly inside a match: re.split on the piece
// cannot see it) do not overlap one another -- then re.split keeps every one of them.  Between
// two kept specials (and before the first, after the last) the cuts split the normal text.
// Overlapping matches (a special that overlaps itself or another) go to the host's
// leftmost-longest resolution instead.
__device__ __forceinline__ size_t cuts_le(const unsigned long long* __restrict__ cuts, size_t nc,
                                          unsigned long long p) {   // how many cuts are <= p
    size_t lo = 0, hi = nc;
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (cuts[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void k_sp_eligible(const unsigned long long* __restrict__ keys, size_t m, const uint32_t* __restrict__ sp_len,
                              const unsigned long long* __restrict__ cuts, size_t nc, uint8_t* __restrict__ elig) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long p = keys[j] >> kSpShift, e = p + sp_len[keys[j] & 0xffffu];
        const size_t i = cuts_le(cuts, nc, p);   // the first cut > p
        elig[j] = (i == nc || cuts[i] >= e) ? 1 : 0;
    }
}

// entry j <= me: the segments ending with special j (j == me: the tail after the last one)
__global__ void k_sp_count(const unsigned long long* __restrict__ keys, size_t me, const uint32_t* __restrict__ sp_len,
                           const unsigned long long* __restrict__ cuts, size_t nc, unsigned long long n,
                           unsigned long long* __restrict__ cnt, unsigned* __restrict__ conflict) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j <= me; j += (size_t)gridDim.x * blockDim.x) {
        unsigned long long prev = 0;
        if (j > 0) prev = (keys[j - 1] >> kSpShift) + sp_len[keys[j - 1] & 0xffffu];
        const unsigned long long p = j < me ? keys[j] >> kSpShift : n;
        if (p < prev) atomicOr(conflict, 1u);
        unsigned long long c = j < me ? 1 : 0;
        if (prev < p) c += 1 + (cuts_le(cuts, nc, p - 1) - cuts_le(cuts, nc, prev));   // cuts in (prev, p)
        cnt[j] = c;
    }
}

__global__ void k_sp_emit(const unsigned long long* __restrict__ keys, size_t me, const uint32_t* __restrict__ sp_len,
                          const unsigned long long* __restrict__ cuts, size_t nc, unsigned long long n,
                          const unsigned long long* __restrict__ off, Seg* __restrict__ segs) {
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j <= me; j += (size_t)gridDim.x * blockDim.x) {
        unsigned long long prev = 0;
        if (j > 0) prev = (keys[j - 1] >> kSpShift) + sp_len[keys[j - 1] & 0xffffu];
        const unsigned long long p = j < me ? keys[j] >> kSpShift : n;
        unsigned long long o = off[j];
        if (prev < p) {
            unsigned long long start = prev;
            for (size_t i = cuts_le(cuts, nc, prev); i < nc && cuts[i] < p; ++i) {
                segs[o++] = Seg{start, cuts[i], -1, 0};
                start = cuts[i];
            }
            segs[o++] = Seg{start, p, -1, 0};
        }
        if (j < me) {
            const unsigned k = (unsigned)(keys[j] & 0xffffu);
            segs[o] = Seg{p, p + sp_len[k], (int)k, 0};
        }
    }
}

// ------------------------------------------------------------------ 2. the scan: one record per pre-token
// Records.  Every pre-token becomes one u32; its top bits say what it names:
//   0 | pw                (scan output only) a word the scan left to k_enc_resolve: pending entry
//                         pw (31 bits), which the resolve overwrites with the word's ids' info
//                         (a dictionary word) or its slot record (resolved_is_rec)
//   kRecDirect | id       11: a word of exactly one vocab id (< 2^30): one-byte words (the byte
//                         table) and the dictionary's one-id words
//   kRecSpecial | k       101: special token k
//   kRecSlot | p          100: p < cap: a word-table slot (a word first met in this text, encoded
//                         after the scan by k_encode_words); cap + s: dictionary slot s (a word of
//                         several ids, or none)
// The dictionary (built once per tokenizer, build_dictionary) holds every vocab entry of 2..16
// bytes with its encoding: a pre-token's ids depend only on its bytes (tokenizer.py:124-136), so
// a word found there needs no word-table entry.  The scan itself touches no global table: a word
// its LDS cache does not hold becomes a pending entry (its position and length, 8 bytes), and a
// separate kernel with registers to spare resolves all of them with many lookups in flight --
// the dictionary (2 MB, L2-resident) first, then the word table.
constexpr uint32_t kRecPendBit = 0x80000000u;   // clear: a pending entry
constexpr uint32_t kRecDirect = 0xC0000000u;
constexpr uint32_t kRecSpecial = 0xA0000000u;
constexpr uint32_t kRecSlot = 0x80000000u;
constexpr uint32_t kRecKind3 = 0xE0000000u;     // the kind of a special / slot record
constexpr uint32_t kRecPayload = 0x3FFFFFFFu;   // direct ids are below this
constexpr uint32_t kRecPayload29 = 0x1FFFFFFFu; // slots and special indices
constexpr uint32_t kRecPendMax = 0x7FFFFFFFu;   // pending entries are below this
constexpr uint32_t kRecNone = 0xFFFFFFFFu;      // byte table / dictionary lookup: no record
constexpr uint32_t kDictMark = 0x40000000u;     // DictEnt.rec of a several-id word: kDictMark | slot
__device__ __forceinline__ bool rec_is_direct(uint32_t r) { return (r & kRecDirect) == kRecDirect; }
// A pending entry after the resolve holds either its word's ids' info (a dictionary word: the
// info format of section 5, never in [2^31, 2^32)) or a record kRecSlot | slot (a word-table
// word, whose ids exist only after k_encode_words; k_enc_finalize swaps it for the info).
__device__ __forceinline__ bool resolved_is_rec(unsigned long long v) { return (v >> 31) == 1; }

// ids' info (section 5): kOneId | id, kTwoIds | id1 << 31 | id0, kThreeIds (ids < 2^20),
// kFourIds (ids < 2^15), else nids << 36 | pool offset
constexpr unsigned long long kOneId = 1ULL << 63;
constexpr unsigned long long kTwoIds = 1ULL << 62;
constexpr unsigned long long kThreeIds = 1ULL << 61;
constexpr unsigned long long kFourIds = 1ULL << 60;
constexpr unsigned long long kInlineIds = kOneId | kTwoIds | kThreeIds | kFourIds;
constexpr int kNidsShift = 36;
constexpr unsigned long long kDictPool = 1ULL << 35;
constexpr unsigned long long kPoolOff = kDictPool - 1;

struct DictEnt {               // 32 bytes: one probe is one aligned 32-byte read
    uint64_t lo, hi;           // packed bytes
    uint32_t len;              // 0: an empty slot
    uint32_t rec;              // the word's record (kRecDirect | id, or kDictMark | this slot)
    unsigned long long info;   // its ids (slot_info format below; the pool is the dictionary's)
};
struct EncDict {
    const DictEnt* ent;
    unsigned long long mask;   // slots - 1
    const uint32_t* pool;
    const uint32_t* byte_rec;  // 256 records of the one-byte words (kRecNone: through the table)
    const uint32_t* filt;      // membership bits: a word whose bit is clear is not in the dictionary
};
// The dictionary's membership filter: one bit per hash value's bits 20..39 (128 KB, which stays
// in every XCD's L2 where the 2 MB of entries do not: the resolve's table words, 63 % of the
// pending words at the bench corpus, mostly skip the dictionary probe that would miss L2)
constexpr int kFiltShift = 20;
constexpr unsigned kFiltBits = 1u << 20;
__host__ __device__ inline unsigned filt_index(uint64_t h) { return (unsigned)(h >> kFiltShift) & (kFiltBits - 1); }
__device__ __forceinline__ bool filt_maybe(const EncDict& D, uint64_t h) {
    const unsigned i = filt_index(h);
    return (D.filt[i >> 5] >> (i & 31)) & 1u;
}

__device__ __forceinline__ uint32_t dict_find(const EncDict& D, uint64_t wl, uint64_t wh, uint32_t len, uint64_t h) {
    if (!filt_maybe(D, h)) return kRecNone;
    size_t sl = h & D.mask;
    for (;;) {
        const DictEnt e = D.ent[sl];
        if (e.len == 0) return kRecNone;
        if (e.len == len && e.lo == wl && e.hi == wh) return e.rec;
        sl = (sl + 1) & D.mask;
    }
}
// the same, answering with the word's ids' info (the resolve stores it in the pending entry, so a
// dictionary word needs nothing more after the resolve)
__device__ __forceinline__ bool dict_find_info(const EncDict& D, uint64_t wl, uint64_t wh, uint32_t len, uint64_t h,
                                               unsigned long long* info) {
    if (!filt_maybe(D, h)) return false;
    size_t sl = h & D.mask;
    for (;;) {
        const DictEnt e = D.ent[sl];
        if (e.len == 0) return false;
        if (e.len == len && e.lo == wl && e.hi == wh) {
            *info = e.info;
            return true;
        }
        sl = (sl + 1) & D.mask;
    }
}

// LDS word cache of the scan (2-way): word -> record (build knob BPE355_ENC_CACHE, a power of 2)
#ifndef BPE355_ENC_CACHE
#define BPE355_ENC_CACHE 512
#endif
constexpr int kEncCache = BPE355_ENC_CACHE;
static_assert((kEncCache & (kEncCache - 1)) == 0, "the scan's cache size is a power of two");
#ifndef BPE355_ENC_EPOCH
#define BPE355_ENC_EPOCH 4
#endif
constexpr int kEncEpoch = BPE355_ENC_EPOCH;   // chunks between the scan cache's evictions
constexpr unsigned kEncKeep = 2;
constexpr int kSegLds = 64;

__device__ __forceinline__ int seg_of(const Seg* __restrict__ segs, int nseg, size_t p) {
    int lo = 0, hi = nseg - 1;  // last segment with start <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].start <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct ClipWin {   // one block's window with the bytes before window position lo read as '\n'
    int r0, lo;
    __device__ __forceinline__ uint32_t byte(int j) const { return j < lo ? 0x0Au : g_stage[r0 + j]; }
    __device__ __forceinline__ uint32_t dword(int k) const {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(g_stage + r0 + 4 * k);
        const int q = lo - 4 * k;   // bytes of this dword before the segment start
        if (q <= 0) return x;
        if (q >= 4) return 0x0A0A0A0Au;
        const uint32_t m = (1u << (8 * q)) - 1u;
        return (x & ~m) | (0x0A0A0A0Au & m);
    }
};

// The encoder's word table, over the training table's arrays (kv: 16-byte entries, pos): the
// encoder counts nothing, so an entry's second word holds the word's first 8 bytes and a probe
// is one 16-byte load, with no read of the text to verify a key:
//   words of <= 15 bytes: kv[2s] = kInl | len << 56 | bytes 8..14, kv[2s + 1] = ~(bytes 0..7)
//     (claimed by a CAS on the first word, then the second stored; it is never 0 -- that would
//     take eight 0xFF bytes, which valid UTF-8 never holds -- so 0 means "not stored yet" and
//     matches no word, not even one of NUL bytes.  A reader that sees the first word before the
//     second may miss the word and insert it again further on -- a duplicate slot, which encodes
//     to the same ids);
//   longer words: kv[2s] = len << 40 | (offset + 1) of an occurrence, verified against the text.
// pos[s] = an occurrence's offset (k_collect reads (offset, len) of every slot as before).
constexpr int kEncInline = 15;

__device__ __forceinline__ size_t enc_table_add(const uint8_t* __restrict__ s, size_t gp, size_t len, uint64_t wl,
                                                uint64_t wh, uint64_t h, unsigned long long* __restrict__ kv,
                                                unsigned long long* __restrict__ pos, size_t mask,
                                                unsigned* __restrict__ status, bool* inserted) {
    *inserted = false;
    const bool inl = len <= (size_t)kEncInline;
    const unsigned long long mine = inl ? kInl | ((unsigned long long)len << 56) | wh
                                        : ((unsigned long long)len << 40) | (gp + 1);
    size_t slot = h & mask;
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(kv + 2 * slot);
        unsigned long long k = e.x, k0 = e.y;
        if (k == 0) {
            k = atomicCAS(&kv[2 * slot], 0ULL, mine);
            if (k == 0) {   // claimed
                if (inl) kv[2 * slot + 1] = ~wl;
                pos[slot] = gp;
                *inserted = true;
                return slot;
            }
            k0 = kv[2 * slot + 1];
        }
        if (inl) {
            if (k == mine && k0 == ~wl) return slot;
        } else if (!(k & kInl) && (k >> 40) == len) {
            const size_t q = (k & kOffMask) - 1;
            if (bytes_equal(s, q, gp, len)) return slot;
        }
        slot = (slot + 1) & mask;
    }
    atomicOr(status, 1u);
    return ~(size_t)0;
}


struct ScanArgs {
    const uint8_t* s;
    size_t n, n_chunks;
    const Seg* segs;
    int nseg, use_cache;
    unsigned long long* kv;           // the word table (stage.h)
    unsigned long long* pos;
    size_t mask;
    unsigned long long max_fill;
    unsigned long long* fill;
    uint32_t* recs;                   // records, each chunk's run contiguous
    unsigned long long rec_cap;
    unsigned long long rec_region;    // records a workgroup reserves at a time (>= kChunk)
    unsigned long long* rec_fill;
    unsigned long long* rec_base;     // per chunk: its run in recs
    uint32_t* rec_n;
    unsigned long long* pend;         // pending entries: position << 24 | length
    unsigned pend_blocks;             // blocks of kPendBlock entries in the pool
    unsigned* pend_nblk;              // blocks handed out
    uint32_t* block_used;             // entries used per block
    unsigned* status;
};

// The optional export of the scan (encode_batch): for every cut -- a document start inside the
// text -- the index, inside its chunk's record run, of the token that starts there.
struct ScanCuts {
    const unsigned long long* cuts;   // sorted, distinct, in (0, n)
    const uint32_t* chunk_cut0;       // n_chunks + 1: the first cut at or after each chunk's first byte
    uint32_t* cut_rec;                // per cut: record index inside its chunk's run
};
// The export of the span calls (encode with offsets), on top of the cuts': every record's first
// byte, relative to its chunk (< kChunk, so 16 bits), at the record's index in an array parallel
// to recs.
struct ScanCutsPos : ScanCuts {
    uint16_t* rec_pos;
};
static_assert(kChunk <= 65536, "a record's chunk-relative position fits 16 bits");

// A workgroup appends its pending entries to a block of the pool it holds; a block is
// chunk-sized (a chunk has at most one pre-token per byte), so a chunk that does not fit the
// rest of the block takes a new one before its token phase and the appends never check.
constexpr unsigned kPendBlock = kChunk;
constexpr int kPendShift = 24;        // pending entry: position << 24 | length (< 2^24)

// a dictionary record as the emit reads it: several-id words are cap + their dictionary slot
__device__ __forceinline__ uint32_t dict_rec(uint32_t rec, size_t cap) {
    return (rec & kRecDirect) == kDictMark ? kRecSlot | (uint32_t)(cap + (rec & kRecPayload)) : rec;
}

// Persistent workgroups stream 16 KiB chunks through LDS (stage2.h).  Every thread turns its
// 64-byte block into a token-start mask with tokstart.h's predicate, evaluated once per segment
// that overlaps the block on a window clipped to that segment (bytes before the segment start
// read '\n', the segment end is the text end: each segment is pre-tokenized on its own,
// tokenizer.py:68-90); a special segment is one token.  A block's pre-tokens are the set bits of
// its mask, so the chunk's record count and every thread's offset in the chunk's run are one
// block scan of popcounts, and the records of a chunk are written densely.  Per pre-token: a
// special or a one-byte word is its record; a word of 2..16 bytes is looked up in the LDS cache
// (word -> record); anything else becomes a pending entry, cached as such.  Only when the pool
// of pending entries is spent does the scan resolve words itself (dictionary, word table).
// workgroups per CU the scan's registers are capped for (build knob)
#ifndef BPE355_ENC_SCAN_WG
#define BPE355_ENC_SCAN_WG 4
#endif
// the scan's next-chunk loads before the mask phase: 35 spilled VGPRs instead of 63, but no faster
// (168.6-169.4 vs 168.6-168.7 ms per encode, profiles/r04/y_*), so off
#ifndef BPE355_ENC_EARLY_PREFETCH
#define BPE355_ENC_EARLY_PREFETCH 0
#endif
// kCuts: the instantiations of encode_batch also export every cut's record index (ScanCuts); in the
// others C is never read.  kPos: the span calls' instantiations (always with kCuts) also export
// every record's position (ScanCutsPos); the others take a plain ScanCuts and are unchanged.
template <bool kAligned, bool kCuts, bool kPos = false>
__global__ void __launch_bounds__(256, BPE355_ENC_SCAN_WG)
k_enc_scan4(ScanArgs A, EncDict D, typename std::conditional<kPos, ScanCutsPos, ScanCuts>::type C) {
    __shared__ uint64_t s_mask[kWords];
    __shared__ unsigned long long c_key[kEncCache];
    __shared__ uint64_t c_lo[kEncCache], c_hi[kEncCache];
    __shared__ uint32_t c_rec[kEncCache];
    __shared__ uint16_t c_hit[kEncCache];   // hits this epoch
    __shared__ uint32_t s_brec[256];
    __shared__ Seg s_seg[kSegLds];
    __shared__ int s_seg0, s_segn;   // first segment of the chunk window and how many are in LDS (-1: too many)
    __shared__ unsigned long long s_red[4];
    __shared__ uint32_t s_wsum[4];
    __shared__ unsigned long long s_rbase, s_rnext, s_rend;   // the record region the workgroup holds
    __shared__ int s_stop, s_pblk;   // s_pblk: the pending block held (-2: none yet, -1: pool spent)
    __shared__ unsigned s_pused;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* __restrict__ s = A.s;
    const size_t n = A.n;
    const size_t cap = A.mask + 1;
    for (int i = tid; i < kEncCache; i += blockDim.x) { c_key[i] = 0; c_hit[i] = 0; }
    s_brec[tid] = D.byte_rec[tid];
    if (tid == 0) {
        s_pblk = A.pend ? -2 : -1;
        s_pused = 0;
        s_rnext = s_rend = 0;
    }
    load_cls2(tid, blockDim.x);
    unsigned long long inserted = 0;

    // a word resolved here (the pool is spent): dictionary, then the word table (its slot; 0 when
    // the table is full: the host retries with a larger one)
    auto resolve_here = [&](size_t len, size_t gp, uint64_t wl, uint64_t wh, uint64_t h) -> uint32_t {
        if (len <= (size_t)kInline && len >= 2) {
            const uint32_t rec = dict_find(D, wl, wh, (uint32_t)len, h);
            if (rec != kRecNone) return dict_rec(rec, cap);
        }
        bool ins = false;
        const size_t slot = enc_table_add(s, gp, len, wl, wh, h, A.kv, A.pos, A.mask, A.status, &ins);
        inserted += ins;
        return kRecSlot | (slot == ~(size_t)0 ? 0u : (uint32_t)slot);
    };
    // a word left to k_enc_resolve, or resolved here when the pool is spent
    auto pending = [&](size_t len, size_t gp, uint64_t wl, uint64_t wh, bool packed) -> uint32_t {
        const int pb = s_pblk;
        if (pb >= 0) {
            const unsigned idx = atomicAdd(&s_pused, 1u);   // < kPendBlock: reserved per chunk
            const unsigned long long pw = (unsigned long long)pb * kPendBlock + idx;
            A.pend[pw] = ((unsigned long long)gp << kPendShift) | len;
            return (uint32_t)pw;   // a pending record: bit 31 clear
        }
        if (!packed && len <= (size_t)kInline) pack_word(s, gp, len, wl, wh);
        const uint64_t h = len <= (size_t)kInline ? short_hash(wl, wh, len) : hash_word(s, gp, len);
        return resolve_here(len, gp, wl, wh, h);
    };
    // a pre-token of 2..16 bytes at stage position r (global gp): the LDS cache, else pending
    auto short_rec = [&](uint32_t r, size_t len, size_t gp) -> uint32_t {
        uint64_t wl, wh;
        pack_stage(kPre + (int)r, (int)len, wl, wh);
        const uint64_t h = short_hash(wl, wh, len);
        const unsigned ls = (unsigned)(h >> 40) & (kEncCache - 2);
        if (A.use_cache) {
            for (int way = 0; way < 2; ++way) {
                const unsigned sl = ls + way;
                const unsigned long long k = c_key[sl];
                if (k != 0 && k != kBusy && (k >> 40) == len) {
                    __asm__ volatile("" ::: "memory");
                    if (c_lo[sl] == wl && c_hi[sl] == wh) {
                        c_hit[sl] = (uint16_t)(c_hit[sl] + 1);   // a heuristic: races may drop hits
                        return c_rec[sl];
                    }
                }
            }
        }
        const uint32_t rec = pending(len, gp, wl, wh, true);
        if (A.use_cache) {
            for (int way = 0; way < 2; ++way) {   // cache it if a way is free
                const unsigned sl = ls + way;
                if (c_key[sl] == 0 && atomicCAS(&c_key[sl], 0ULL, kBusy) == 0) {
                    c_lo[sl] = wl;
                    c_hi[sl] = wh;
                    c_rec[sl] = rec;
                    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    atomicExch(&c_key[sl], ((unsigned long long)len << 40) | (gp + 1));
                    break;
                }
            }
        }
        return rec;
    };

    uint4 pre[kSVec];
    if (blockIdx.x < A.n_chunks) fetch2<kAligned>(pre, s, n, (size_t)blockIdx.x * kChunk, tid);
    for (size_t c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
        __syncthreads();
        store2(pre, tid);
        const size_t base = c * kChunk;
        if (tid < 64) {   // wave 0: the segments that overlap the staged window, into LDS
            const size_t w0 = base >= (size_t)kPre ? base - kPre : 0, w1 = base + kWin + kPost;
            const int k0 = seg_of(A.segs, A.nseg, w0);
            const int i = k0 + tid;
            Seg sg{};
            if (i < A.nseg) sg = A.segs[i];
            const bool in = i < A.nseg && sg.start < w1;
            if (in) s_seg[tid] = sg;
            const unsigned long long b = __ballot(in);
            if (tid == 0) {
                s_seg0 = k0;
                s_segn = (b == ~0ULL && k0 + 64 < A.nseg && A.segs[k0 + 64].start < w1) ? -1 : __popcll(b);
                s_stop = *(volatile unsigned long long*)A.fill > A.max_fill;
            }
        }
        __syncthreads();
        if (s_stop) {
            if (tid == 0) atomicOr(A.status, 1u);
            break;
        }
        // the next chunk's loads: before the mask phase (build knob BPE355_ENC_EARLY_PREFETCH), so
        // that they land during its VALU work instead of stalling the token phase's first wait
        if (BPE355_ENC_EARLY_PREFETCH && c + gridDim.x < A.n_chunks) fetch2<kAligned>(pre, s, n, (c + gridDim.x) * kChunk, tid);
        const int seg0 = s_seg0, segn = s_segn;
        auto seg_at = [&](int i) -> Seg { return segn >= 0 ? s_seg[i - seg0] : A.segs[i]; };
        const int seg_end = segn >= 0 ? seg0 + segn : A.nseg;
        auto seg_find = [&](size_t p) -> int {   // the segment holding position p
            if (segn < 0) return seg_of(A.segs, A.nseg, p);
            int lo = seg0, hi = seg_end - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_seg[mid - seg0].start <= p) lo = mid;
                else hi = mid - 1;
            }
            return lo;
        };

        // ---- token starts of this thread's block, per overlapping segment
        const size_t blk = base + 64 * (size_t)tid;
        uint64_t starts = 0, spec = 0;
        if (blk < n) {
            const long long wstart = (long long)blk - kStartPre;
            const int r0 = kPre + 64 * tid - kStartPre;
            for (int i = seg_find(blk); i < seg_end; ++i) {
                const Seg sg = seg_at(i);
                if (sg.start >= blk + 64) break;
                if (sg.end <= blk) continue;
                if (sg.special >= 0) {
                    if (sg.start >= blk) {
                        starts |= 1ULL << (sg.start - blk);
                        spec |= 1ULL << (sg.start - blk);
                    }
                    continue;
                }
                const long long lo = (long long)sg.start - wstart, hi = (long long)sg.end - wstart;
                uint64_t m = token_starts64<DevTab>(ClipWin{r0, lo > 0 ? (int)lo : 0},
                                                    (int)(hi < kStartWin ? hi : kStartWin));
                const int a = sg.start > blk ? (int)(sg.start - blk) : 0;
                const int e = sg.end < blk + 64 ? (int)(sg.end - blk) : 64;
                m &= (e >= 64 ? ~0ULL : ((1ULL << e) - 1)) & (~0ULL << a);
                if (sg.start >= blk) m |= 1ULL << a;   // the segment starts a token
                starts |= m;
            }
        }
        s_mask[tid] = starts;
        // the thread's offset in the chunk's run: a block scan of the per-block record counts
        const uint32_t cnt = (uint32_t)__popcll(starts);
        uint32_t x = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wsum[wave] = x;
        if (!BPE355_ENC_EARLY_PREFETCH && c + gridDim.x < A.n_chunks) fetch2<kAligned>(pre, s, n, (c + gridDim.x) * kChunk, tid);
        __syncthreads();
        uint32_t toff = x - cnt;
        for (int w = 0; w < wave; ++w) toff += s_wsum[w];
        if (kCuts) {   // the cuts in this block: a token starts at each (a cut ends every segment)
            uint32_t lo = C.chunk_cut0[c];
            const uint32_t q1 = C.chunk_cut0[c + 1];
            for (uint32_t hi = q1; lo < hi;) {   // the first cut at or after blk
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (C.cuts[mid] < blk) lo = mid + 1;
                else hi = mid;
            }
            for (; lo < q1; ++lo) {
                const unsigned long long d = C.cuts[lo] - blk;
                if (d >= 64) break;
                C.cut_rec[lo] = toff + (uint32_t)__popcll(starts & ((1ULL << d) - 1));
            }
        }
        if (tid == 0) {
            const uint32_t total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
            // the chunk's run in the workgroup's region; a new region (one global reservation per
            // rec_region records) when it does not fit
            unsigned long long b = s_rnext;
            if (b + total > s_rend) {
                b = atomicAdd(A.rec_fill, A.rec_region);
                s_rend = b + A.rec_region;
                if (s_rend > A.rec_cap) {   // the record buffer is too small: the host retries
                    atomicOr(A.status, 256u);
                    s_rend = 0;
                    b = ~0ULL;
                }
            }
            if (b != ~0ULL) s_rnext = b + total;
            s_rbase = b;
            A.rec_base[c] = b == ~0ULL ? 0 : b;
            A.rec_n[c] = b == ~0ULL ? 0 : total;
            // room in the pending block for every pre-token of the chunk
            if (s_pblk != -1 && (s_pblk == -2 || s_pused + total > kPendBlock)) {
                if (s_pblk >= 0) A.block_used[s_pblk] = s_pused;
                const unsigned nb = atomicAdd(A.pend_nblk, 1u);
                s_pblk = nb < A.pend_blocks ? (int)nb : -1;
                s_pused = 0;
            }
        }
        __syncthreads();
        const unsigned long long rbase = s_rbase;

        // ---- one record per pre-token that starts in the block
        if (rbase != ~0ULL) {
            uint32_t* const out = A.recs + rbase + toff;
            const size_t rem = n > base ? n - base : 0;
            const uint32_t tend = rem < (size_t)kWin ? (uint32_t)rem : (uint32_t)kWin;
            uint32_t k = 0;
            uint64_t m = starts;
            while (m) {
                const uint32_t j = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                const uint32_t r = 64u * tid + j;
                const size_t gp = base + r;
                uint32_t rec;
                if ((spec >> j) & 1ULL) {
                    rec = kRecSpecial | (uint32_t)seg_at(seg_find(gp)).special;
                } else {
                    size_t e;   // end (global)
                    if (m) {
                        e = base + 64u * tid + (uint32_t)__builtin_ctzll(m);
                    } else {
                        e = ~(size_t)0;
                        for (int w = tid + 1; w < kWords; ++w) {
                            const uint64_t xw = s_mask[w];
                            if (xw) { e = base + 64u * w + (uint32_t)__builtin_ctzll(xw); break; }
                        }
                        if (e == ~(size_t)0) {   // the chunk's last pre-token: its segment decides
                            const Seg sg = seg_at(seg_find(gp));
                            const size_t lim = sg.end < base + tend ? sg.end : base + tend;
                            e = base + token_end(StageText{}, (uint32_t)(lim - base), r);
                            if (lim != sg.end && e + 4 > lim) e = token_end(s, (size_t)sg.end, gp);
                        }
                    }
                    if (e <= gp) { atomicOr(A.status, 16u); rec = kRecSlot; }
                    else {
                        const size_t len = e - gp;
                        if (len == 1) {
                            rec = s_brec[StageText{}[r]];
                            if (rec == kRecNone) rec = pending(1, gp, 0, 0, false);
                        } else if (len <= (size_t)kInline) {
                            rec = short_rec(r, len, gp);
                        } else if (len >= kMaxPretok) {
                            atomicOr(A.status, 2u);
                            rec = kRecSlot;
                        } else {
                            rec = pending(len, gp, 0, 0, false);
                        }
                    }
                }
                if constexpr (kPos) C.rec_pos[rbase + toff + k] = (uint16_t)r;
                out[k++] = rec;
            }
        }
        if ((c - blockIdx.x) / gridDim.x % kEncEpoch == kEncEpoch - 1) {   // cache eviction
            __syncthreads();
            for (int i = tid; i < kEncCache; i += blockDim.x) {
                const unsigned long long kk = c_key[i];
                if (kk == 0 || kk == kBusy) continue;
                if (c_hit[i] >= kEncKeep) { c_hit[i] = 0; continue; }
                c_key[i] = 0;
                c_hit[i] = 0;
            }
        }
        const unsigned long long ins = wave_sum(inserted);
        inserted = 0;
        if (lane == 0) s_red[wave] = ins;
        __syncthreads();
        if (tid == 0) {
            const unsigned long long b = s_red[0] + s_red[1] + s_red[2] + s_red[3];
            if (b) atomicAdd(A.fill, b);
        }
    }
    __syncthreads();
    if (tid == 0 && s_pblk >= 0) A.block_used[s_pblk] = s_pused;
}

// Every pending entry to its final record, in place: the word's bytes from the text, then the
// dictionary, then the word table.  One entry per thread, no mask work: the lookups of many
// entries are in flight at once.
struct ResolveArgs {
    const uint8_t* s;
    size_t n;
    unsigned long long* pend;
    const uint32_t* block_used;
    unsigned long long n_entries;     // blocks handed out x kPendBlock
    unsigned long long* kv;
    unsigned long long* pos;
    size_t mask;
    unsigned long long max_fill;      // words the table takes (load 1/2) before the host retries
    unsigned long long* fill;
    unsigned* status;
    unsigned long long* stats;        // BPE355_TRACE: LDS-cache hits, dictionary hits, table words; else null
};

// the resolve's counters (trace only): one atomic per wave and counter
__device__ __forceinline__ void resolve_stats(unsigned long long* stats, unsigned long long c0, unsigned long long c1,
                                              unsigned long long c2) {
    if (!stats) return;
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    c2 = wave_sum(c2);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&stats[0], c0);
        atomicAdd(&stats[1], c1);
        atomicAdd(&stats[2], c2);
    }
}

__global__ void __launch_bounds__(256) k_enc_resolve(ResolveArgs A, EncDict D) {
    unsigned long long inserted = 0, n_dict = 0, n_table = 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < A.n_entries; i += stride) {
        if ((i & (kPendBlock - 1)) >= A.block_used[i / kPendBlock]) continue;
        const unsigned long long e = A.pend[i];
        const size_t gp = (size_t)(e >> kPendShift), len = (size_t)(e & ((1ULL << kPendShift) - 1));
        unsigned long long val = 0;
        bool found = false;
        uint64_t wl = 0, wh = 0, h;
        if (len <= (size_t)kInline) {
            load_word(A.s, A.n, gp, len, wl, wh);
            h = short_hash(wl, wh, len);
            if (len >= 2) found = dict_find_info(D, wl, wh, (uint32_t)len, h, &val);
        } else {
            h = hash_word(A.s, gp, len);
        }
        n_dict += found;
        if (!found) {   // (a probe chain past kMaxProbe sets status 1: the host retries)
            bool ins = false;
            const size_t slot = enc_table_add(A.s, gp, len, wl, wh, h, A.kv, A.pos, A.mask, A.status, &ins);
            inserted += ins;
            ++n_table;
            val = kRecSlot | (slot == ~(size_t)0 ? 0u : (uint32_t)slot);
        }
        A.pend[i] = val;
    }
    resolve_stats(A.stats, 0, n_dict, n_table);
    inserted = wave_sum(inserted);
    if ((threadIdx.x & 63) == 0 && inserted) atomicAdd(A.fill, inserted);
}

// The same with an LDS word cache: a workgroup takes the scan's blocks one at a time (a block
// holds one scan workgroup's misses over ~16 chunks, where mid-frequency words recur beyond the
// scan's small cache), and a word met again skips the dictionary and the table.
constexpr int kResCache = 1024;
__global__ void __launch_bounds__(256) k_enc_resolve_c(ResolveArgs A, EncDict D, unsigned n_blocks) {
    __shared__ unsigned long long c_key[kResCache];
    __shared__ uint64_t c_lo[kResCache], c_hi[kResCache];
    __shared__ uint32_t c_rec[kResCache];   // kRecDirect | id (a one-id dictionary word) or kRecSlot | slot
    unsigned long long inserted = 0, n_hit = 0, n_dict = 0, n_table = 0;
    for (int i = threadIdx.x; i < kResCache; i += blockDim.x) c_key[i] = 0;
    __syncthreads();
    __shared__ unsigned long long s_ins;
    __shared__ int s_full;
    for (unsigned b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        // the words this workgroup inserted so far go to the fill count; past the table's
        // half-load the resolve stops (the host retries with a 4 x larger table)
        const unsigned long long ins = wave_sum(inserted);
        inserted = 0;
        if (threadIdx.x == 0) { s_ins = 0; s_full = 0; }
        __syncthreads();
        if ((threadIdx.x & 63) == 0 && ins) atomicAdd(&s_ins, ins);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long f = s_ins ? atomicAdd(A.fill, s_ins) + s_ins : *(volatile unsigned long long*)A.fill;
            if (f > A.max_fill) {
                s_full = 1;
                atomicOr(A.status, 1u);
            }
        }
        __syncthreads();
        if (s_full) return;
        const unsigned used = A.block_used[b];
        const size_t base = (size_t)b * kPendBlock;
        for (unsigned j = threadIdx.x; j < used; j += blockDim.x) {
            const unsigned long long e = A.pend[base + j];
            const size_t gp = (size_t)(e >> kPendShift), len = (size_t)(e & ((1ULL << kPendShift) - 1));
            unsigned long long val = 0;   // the dictionary word's info, or the table word's record
            bool found = false;
            uint64_t wl = 0, wh = 0, h;
            unsigned ls = 0;
            const bool cacheable = len >= 2 && len <= (size_t)kInline;
            if (len <= (size_t)kInline) {
                load_word(A.s, A.n, gp, len, wl, wh);
                h = short_hash(wl, wh, len);
                if (cacheable) {
                    ls = (unsigned)(h >> 40) & (kResCache - 2);
                    for (int way = 0; way < 2 && !found; ++way) {
                        const unsigned sl = ls + way;
                        const unsigned long long k = c_key[sl];
                        if (k != 0 && k != kBusy && (k >> 40) == len) {
                            __asm__ volatile("" ::: "memory");
                            if (c_lo[sl] == wl && c_hi[sl] == wh) {
                                const uint32_t r = c_rec[sl];
                                val = rec_is_direct(r) ? kOneId | (r & kRecPayload) : r;
                                found = true;
                            }
                        }
                    }
                    if (found) {
                        ++n_hit;
                        A.pend[base + j] = val;
                        continue;
                    }
                    found = dict_find_info(D, wl, wh, (uint32_t)len, h, &val);
                    n_dict += found;
                }
            } else {
                h = hash_word(A.s, gp, len);
            }
            if (!found) {   // (a probe chain past kMaxProbe sets status 1: the host retries)
                bool ins = false;
                const size_t slot = enc_table_add(A.s, gp, len, wl, wh, h, A.kv, A.pos, A.mask, A.status, &ins);
                inserted += ins;
                ++n_table;
                val = kRecSlot | (slot == ~(size_t)0 ? 0u : (uint32_t)slot);
            }
            // cache it if a way is free (a table word's slot or a one-id word's id; a dictionary
            // word of several ids, rare, is not cached)
            const bool one = (val & kOneId) && (uint32_t)val < kRecPayload;
            if (cacheable && (one || resolved_is_rec(val))) {
                for (int way = 0; way < 2; ++way) {
                    const unsigned sl = ls + way;
                    if (c_key[sl] == 0 && atomicCAS(&c_key[sl], 0ULL, kBusy) == 0) {
                        c_lo[sl] = wl;
                        c_hi[sl] = wh;
                        c_rec[sl] = one ? kRecDirect | (uint32_t)val : (uint32_t)val;
                        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        atomicExch(&c_key[sl], ((unsigned long long)len << 40) | 1ULL);
                        break;
                    }
                }
            }
            A.pend[base + j] = val;
        }
        if (((b - blockIdx.x) / gridDim.x) % 4 == 3) {   // a fresh cache every 4 blocks
            __syncthreads();
            for (int i = threadIdx.x; i < kResCache; i += blockDim.x) c_key[i] = 0;
            __syncthreads();
        }
    }
    resolve_stats(A.stats, n_hit, n_dict, n_table);
    inserted = wave_sum(inserted);
    if ((threadIdx.x & 63) == 0 && inserted) atomicAdd(A.fill, inserted);
}

// ------------------------------------------------------------------ 3. unique words
// Every word-table slot in use -> (slot, offset, length).  A workgroup takes kCollectPer x 256
// slots (coalesced) and reserves its words' positions with ONE global atomic: one per wave would
// be ~0.26 M returning atomics on one word at a 16 M-slot table, ~3 ms at ~88 per us.
constexpr unsigned kCollectPer = 8;
__global__ void __launch_bounds__(256) k_collect(const unsigned long long* __restrict__ kv,
                                                 const unsigned long long* __restrict__ pos, size_t cap,
                                                 uint32_t* __restrict__ w_slot, unsigned long long* __restrict__ w_off,
                                                 uint32_t* __restrict__ w_len, unsigned* __restrict__ n_words) {
    __shared__ unsigned s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    const size_t s0 = (size_t)blockIdx.x * 256 * kCollectPer + threadIdx.x;
    unsigned long long key[kCollectPer];
    unsigned mine = 0;
#pragma unroll
    for (unsigned u = 0; u < kCollectPer; ++u) {
        const size_t sl = s0 + (size_t)u * 256;
        key[u] = sl < cap ? kv[2 * sl] : 0ULL;
        mine += key[u] != 0;
    }
    __syncthreads();   // s_n initialised
    const unsigned at = mine ? atomicAdd(&s_n, mine) : 0u;   // LDS: this thread's first position
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_n ? atomicAdd(n_words, s_n) : 0u;
    __syncthreads();
    unsigned w = s_base + at;
#pragma unroll
    for (unsigned u = 0; u < kCollectPer; ++u) {
        const unsigned long long k = key[u];
        if (!k) continue;
        const size_t sl = s0 + (size_t)u * 256;
        const bool inl = (k >> 63) != 0;   // key format: enc_table_add
        w_slot[w] = (uint32_t)sl;
        w_off[w] = inl ? pos[sl] : (k & kOff40) - 1;
        w_len[w] = inl ? (uint32_t)((k >> 56) & 0x7f) : (uint32_t)(k >> 40);
        ++w;
    }
}

// ------------------------------------------------------------------ 5. ids, in one pass
// slot_info[slot] (k_encode_words) and a dictionary entry's info: a word's ids in one 8-byte
// cell -- kOneId | id for a word of one id, kTwoIds | id1 << 31 | id0 for two (ids < 2^31),
// kThreeIds | id2 << 40 | id1 << 20 | id0 for three (ids < 2^20), kFourIds | id3 << 45 | id2 << 30 |
// id1 << 15 | id0 for four (ids < 2^15: vocabularies up to 32768, the bench's 32000), so most
// occurrences need no read of the id pool when their ids are written; else nids << 36 | offset
// into an id pool (the dictionary's pool when kDictPool is set), 0
// for none (a pre-token equal to a special)

__host__ __device__ inline unsigned long long make_info(uint32_t nids, const uint32_t* ids, unsigned long long off) {
    if (nids == 1) return kOneId | ids[0];
    if (nids == 2 && ids[0] < 0x80000000u && ids[1] < 0x80000000u)
        return kTwoIds | ((unsigned long long)ids[1] << 31) | ids[0];
    if (nids == 3 && (ids[0] | ids[1] | ids[2]) < (1u << 20))
        return kThreeIds | ((unsigned long long)ids[2] << 40) | ((unsigned long long)ids[1] << 20) | ids[0];
    if (nids == 4 && (ids[0] | ids[1] | ids[2] | ids[3]) < (1u << 15))
        return kFourIds | ((unsigned long long)ids[3] << 45) | ((unsigned long long)ids[2] << 30) |
               ((unsigned long long)ids[1] << 15) | ids[0];
    return nids ? ((unsigned long long)nids << kNidsShift) | off : 0ULL;
}
__host__ __device__ inline uint32_t info_nids(unsigned long long info) {
    return (info & kOneId) ? 1u : (info & kTwoIds) ? 2u : (info & kThreeIds) ? 3u : (info & kFourIds) ? 4u
                                                        : (uint32_t)((info >> kNidsShift) & 0xffffffu);
}
// an inline info's ids (1..4 of them; the pool format is not inline)
__host__ __device__ inline uint32_t info_inline_ids(unsigned long long info, uint32_t* ids) {
    if (info & kOneId) { ids[0] = (uint32_t)info; return 1; }
    if (info & kTwoIds) {
        ids[0] = (uint32_t)info & 0x7fffffffu;
        ids[1] = (uint32_t)(info >> 31) & 0x7fffffffu;
        return 2;
    }
    if (info & kThreeIds) {
        for (int j = 0; j < 3; ++j) ids[j] = (uint32_t)(info >> (20 * j)) & 0xfffffu;
        return 3;
    }
    for (int j = 0; j < 4; ++j) ids[j] = (uint32_t)(info >> (15 * j)) & 0x7fffu;
    return 4;
}

// After k_encode_words: every resolved pending entry's record replaced by its ids' info (u64,
// slot_info format), so the emit reads a pending word's ids with one gather instead of two
// dependent ones.  One entry per thread, like the resolve.
__global__ void __launch_bounds__(256) k_enc_finalize(unsigned long long* __restrict__ pend,
                                                      const uint32_t* __restrict__ block_used,
                                                      unsigned long long n_entries,
                                                      const unsigned long long* __restrict__ slot_info, size_t cap,
                                                      EncDict D, size_t dict_slots, unsigned* __restrict__ status) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_entries; i += stride) {
        if ((i & (kPendBlock - 1)) >= block_used[i / kPendBlock]) continue;
        const unsigned long long v = pend[i];
        if (!resolved_is_rec(v)) continue;   // a dictionary word's info already
        const uint32_t rec = (uint32_t)v;
        const uint32_t p = rec & kRecPayload29;
        unsigned long long info = 0;
        if (rec_is_direct(rec)) info = kOneId | (rec & kRecPayload);
        else if ((rec & kRecKind3) == kRecSlot && p < cap) info = slot_info[p];
        else if ((rec & kRecKind3) == kRecSlot && p - cap < dict_slots) info = D.ent[p - cap].info;
        else atomicOr(status, 32u);   // a record naming nothing: a bug
        pend[i] = info;
    }
}

struct EmitArgs {
    const uint32_t* recs;
    const unsigned long long* rec_base;
    const uint32_t* rec_n;
    size_t n_chunks;
    const unsigned long long* slot_info;   // word-table slot -> ids
    const uint32_t* pool;
    size_t cap;                            // word-table slots
    EncDict D;
    size_t dict_slots;
    unsigned long long* pend;              // pending entries: their records, or (finalized) their ids' info
    int finalized;
    int writeback;                         // the count pass stores the infos it resolves (no finalize pass)
    const int64_t* sp_vid;
    unsigned long long* ctot;              // per chunk part: its ids (the count pass)
    const unsigned long long* coff;        // per chunk part: its first id's position (exclusive scan)
    unsigned* status;
};

// a record's ids in slot_info format (a one-id word carries its id)
__device__ __forceinline__ unsigned long long rec_info(const EmitArgs& A, uint32_t rec, bool wb = false) {
    uint32_t pw = ~0u;
    if (!(rec & kRecPendBit)) {
        const unsigned long long v = A.pend[rec];
        if (A.finalized || !resolved_is_rec(v)) return v;   // the ids' info (finalize or the resolve)
        pw = rec;
        rec = (uint32_t)v;                                  // k_enc_resolve: a table word's record
    }
    unsigned long long info = 0;
    const uint32_t p = rec & kRecPayload29;
    if (rec_is_direct(rec)) info = kOneId | (rec & kRecPayload);
    else if ((rec & kRecKind3) == kRecSpecial) info = kOneId | (uint32_t)A.sp_vid[p];
    else if (p < A.cap) info = A.slot_info[p];
    else if (p - A.cap < A.dict_slots) info = A.D.ent[p - A.cap].info;
    else atomicOr(A.status, 32u);   // a record naming nothing: a bug
    // the count pass of the no-finalize mode: the pending entry takes its info (every record
    // naming it stores the same value), so the write pass reads it directly
    if (wb && pw != ~0u) A.pend[pw] = info;
    return info;
}

// the ids of one info through put(position, id), from position o; returns how many
template <class Put>
__device__ __forceinline__ uint32_t put_ids(const EmitArgs& A, unsigned long long info, uint32_t o, const Put& put) {
    if (info & kInlineIds) {
        uint32_t ids[4];
        const uint32_t nm = info_inline_ids(info, ids);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (j < nm) put(o + j, ids[j]);
        return nm;
    }
    const uint32_t nm = info_nids(info);
    const uint32_t* src = ((info & kDictPool) ? A.D.pool : A.pool) + (info & kPoolOff);
    for (uint32_t j = 0; j < nm; ++j) put(o + j, src[j]);
    return nm;
}

// exclusive scan of v over the 256 threads: this thread's offset; *total = the sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_ws, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_ws[wave] = x;
    __syncthreads();
    uint32_t off = x - v;
    for (int w = 0; w < wave; ++w) off += s_ws[w];
    *total = s_ws[0] + s_ws[1] + s_ws[2] + s_ws[3];
    __syncthreads();
    return off;
}

// Two passes over the chunks, no dependence between workgroups: kCount sums each chunk's ids
// (its records' infos gathered, all loads issued together) into ctot[c]; after an exclusive scan
// of those (coff), the write pass gathers them again -- the chunk's pending entries were just
// read and sit in a few KB of L2 -- assembles the ids in LDS and stores them with coalesced
// 16-byte writes at coff[c] (a chunk averages ~5 K ids).  (A one-pass form with a decoupled
// look-back over the chunks measured slower: its look-back chains)  OutT
// uint32_t: the ids; uint16_t: np.uint16 as encode.py saves them (encode.py:37), an id past
// 65535 reported in status (bit 128) instead of wrapped.
// The passes work on PARTS of chunks (kEmitParts per chunk, the chunk's records split evenly):
// half the registers and LDS of a whole chunk, so twice the workgroups per CU to hide the
// gathers' latency (the write pass is latency-bound at 3 workgroups per CU).
constexpr unsigned kEmitParts = 2;
constexpr unsigned kEmitIds = 12288 / kEmitParts;   // ids staged per part
constexpr int kEmitR = 16 / (int)kEmitParts;        // records per thread held in registers

template <class OutT, bool kCount>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) k_enc_emit(EmitArgs A, OutT* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t buf[kCount ? 4 : kEmitIds];
    __shared__ uint32_t s_ws[4];
    __shared__ unsigned s_wide;
    const int tid = threadIdx.x;
    constexpr bool kNarrow = sizeof(OutT) == 2;
    bool wide = false;
    if (tid == 0) s_wide = 0;
    for (size_t c = blockIdx.x; c < A.n_chunks * kEmitParts; c += gridDim.x) {   // c: a part
        const size_t ch = c / kEmitParts;
        const unsigned part = (unsigned)(c % kEmitParts);
        const uint32_t mc = A.rec_n[ch];
        const uint32_t r0 = (uint32_t)((unsigned long long)mc * part / kEmitParts);
        const uint32_t m = (uint32_t)((unsigned long long)mc * (part + 1) / kEmitParts) - r0;
        const uint32_t* __restrict__ r = A.recs + A.rec_base[ch] + r0;
        if (m <= 256u * kEmitR) {
            const uint32_t R = (m + 255) >> 8;
            const uint32_t lo = tid * R, hi = lo + R < m ? lo + R : m;
            unsigned long long info[kEmitR];
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) info[i] = lo + i < hi ? rec_info(A, r[lo + i], kCount && A.writeback) : 0ULL;
            uint32_t sum = 0;
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) sum += lo + i < hi ? info_nids(info[i]) : 0u;
            uint32_t T;
            const uint32_t toff = block_excl_scan(sum, s_ws, &T);
            if (kCount) {
                if (tid == 0) A.ctot[c] = T;
            } else if (T <= kEmitIds) {
                const unsigned long long P = A.coff[c];
                uint32_t o = toff;
#pragma unroll
                for (int i = 0; i < kEmitR; ++i)
                    if (lo + i < hi) o += put_ids(A, info[i], o, [&](uint32_t q, uint32_t v) { buf[q] = v; });
                __syncthreads();
                // out + P is OutT-aligned: a scalar head up to 16-byte alignment, then 16-byte stores
                constexpr unsigned kPer = 16 / sizeof(OutT);
                const unsigned head = (unsigned)(((16 - ((uintptr_t)(out + P) & 15)) & 15) / sizeof(OutT));
                const unsigned h = head < T ? head : T;
                if ((unsigned)tid < h) {
                    out[P + tid] = (OutT)buf[tid];
                    wide |= buf[tid] > 0xffffu;
                }
                const unsigned body = (T - h) / kPer;
                uint4* dst = reinterpret_cast<uint4*>(out + P + h);
                for (unsigned i = tid; i < body; i += 256) {
                    const unsigned q = h + kPer * i;
                    if (kNarrow) {
                        uint32_t w[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t a = buf[q + 2 * k], b = buf[q + 2 * k + 1];
                            wide |= (a | b) > 0xffffu;
                            w[k] = (a & 0xffffu) | (b << 16);
                        }
                        dst[i] = make_uint4(w[0], w[1], w[2], w[3]);
                    } else {
                        dst[i] = make_uint4(buf[q], buf[q + 1], buf[q + 2], buf[q + 3]);
                    }
                }
                for (unsigned q = h + kPer * body + tid; q < T; q += 256) {
                    out[P + q] = (OutT)buf[q];
                    wide |= buf[q] > 0xffffu;
                }
                __syncthreads();   // buf is reused by the next chunk
            } else {   // too many ids for LDS: straight to memory
                const unsigned long long P = A.coff[c];
                uint32_t o = toff;
#pragma unroll
                for (int i = 0; i < kEmitR; ++i)
                    if (lo + i < hi)
                        o += put_ids(A, info[i], o, [&](uint32_t q, uint32_t v) {
                            out[P + q] = (OutT)v;
                            wide |= kNarrow && v > 0xffffu;
                        });
            }
        } else if (kCount) {   // many records: rounds of 256
            uint32_t sum = 0;
            for (uint32_t b = 0; b < m; b += 256)
                if (b + tid < m) sum += info_nids(rec_info(A, r[b + tid], A.writeback));
            uint32_t T;
            (void)block_excl_scan(sum, s_ws, &T);
            if (tid == 0) A.ctot[c] = T;
        } else {
            const unsigned long long P = A.coff[c];
            uint32_t run = 0;
            for (uint32_t b = 0; b < m; b += 256) {
                const unsigned long long inf = b + tid < m ? rec_info(A, r[b + tid]) : 0ULL;
                uint32_t rt;
                const uint32_t off = block_excl_scan(b + tid < m ? info_nids(inf) : 0u, s_ws, &rt);
                if (b + tid < m)
                    put_ids(A, inf, run + off, [&](uint32_t q, uint32_t v) {
                        out[P + q] = (OutT)v;
                        wide |= kNarrow && v > 0xffffu;
                    });
                run += rt;
            }
        }
    }
    if (kNarrow && !kCount) {
        if (wide) s_wide = 1;
        __syncthreads();
        if (tid == 0 && s_wide) atomicOr(A.status, 128u);
    }
}

// ------------------------------------------------------------------ 5'. id offsets of the cuts
// encode_batch: where the ids of the token at each cut begin in the output.  The scan left every
// cut's record index inside its chunk's run (ScanCuts::cut_rec, increasing with the cut); a cut's
// id offset is coff[part] + the ids of the part's records before that one.  Shaped like the
// emit's count pass: a workgroup takes the chunk parts that hold a cut (the split is the emit's,
// r0 = mc * part / kEmitParts), reads the part's records in rounds of 256 * kEmitR (each thread
// kEmitR consecutive records, their gathers issued together), leaves the exclusive prefix of
// their id counts in LDS and lets every cut of the round pick its entry -- one pass over the
// records however many cuts there are.  It reads the infos the write pass reads (rec_info with
// the write pass's EmitArgs), so it runs after the coff scan in every BPE355_ENC_FINALIZE mode.
constexpr uint32_t kCutRound = 256u * kEmitR;

__global__ void __launch_bounds__(256) k_enc_cut_offsets(EmitArgs A, const uint32_t* __restrict__ chunk_cut0,
                                                         const uint32_t* __restrict__ cut_rec,
                                                         unsigned long long* __restrict__ cut_off) {
    __shared__ uint32_t s_pre[kCutRound];
    __shared__ uint32_t s_ws[4];
    const int tid = threadIdx.x;
    // the first cut of [lo, hi) whose record index is at or past x
    auto first_at = [&](uint32_t lo, uint32_t hi, uint32_t x) -> uint32_t {
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (cut_rec[mid] < x) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    for (size_t c = blockIdx.x; c < A.n_chunks * kEmitParts; c += gridDim.x) {   // c: a part
        const size_t ch = c / kEmitParts;
        const unsigned part = (unsigned)(c % kEmitParts);
        const uint32_t q0 = chunk_cut0[ch], q1 = chunk_cut0[ch + 1];
        if (q0 == q1) continue;   // no cut in this chunk (uniform over the workgroup)
        const uint32_t mc = A.rec_n[ch];
        const uint32_t r0 = (uint32_t)((unsigned long long)mc * part / kEmitParts);
        const uint32_t m = (uint32_t)((unsigned long long)mc * (part + 1) / kEmitParts) - r0;
        uint32_t j = first_at(q0, q1, r0);             // the part's cuts: [j, j1)
        const uint32_t j1 = first_at(j, q1, r0 + m);
        if (j == j1) continue;
        const uint32_t* __restrict__ r = A.recs + A.rec_base[ch] + r0;
        const unsigned long long P = A.coff[c];
        uint32_t run = 0;   // ids of the rounds before this one
        for (uint32_t b = 0; b < m && j < j1; b += kCutRound) {
            const uint32_t lo = b + tid * kEmitR;
            uint32_t nid[kEmitR];
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) nid[i] = lo + i < m ? info_nids(rec_info(A, r[lo + i])) : 0u;
            uint32_t sum = 0;
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) sum += nid[i];
            uint32_t T;
            uint32_t o = block_excl_scan(sum, s_ws, &T);
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) {
                s_pre[tid * kEmitR + i] = o;
                o += nid[i];
            }
            __syncthreads();
            const uint32_t jn = first_at(j, j1, r0 + b + kCutRound);   // the round's cuts: [j, jn)
            for (uint32_t q = j + tid; q < jn; q += 256) {
                const uint32_t k = cut_rec[q] - r0 - b;   // < kCutRound: [j, jn) is this round's
                cut_off[q] = P + run + s_pre[k < kCutRound ? k : kCutRound - 1];
            }
            j = jn;
            run += T;
            __syncthreads();   // s_pre is reused by the next round
        }
    }
}

// every document start's id offset: 0 for a start at byte 0, the id total for one at the text's
// end (and the closing entry), else its cut's offset
constexpr uint32_t kDocAtZero = 0xFFFFFFFFu, kDocAtEnd = 0xFFFFFFFEu;
__global__ void k_enc_doc_offsets(const uint32_t* __restrict__ doc_cut, size_t n, const unsigned long long* __restrict__ cut_off,
                                  const unsigned long long* __restrict__ coff, const unsigned long long* __restrict__ ctot,
                                  size_t n_parts, unsigned long long* __restrict__ out) {
    const unsigned long long total = coff[n_parts - 1] + ctot[n_parts - 1];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        // doc_cut null: no empty document, so document i > 0 starts at cut i - 1
        const uint32_t k = doc_cut ? doc_cut[i] : i == 0 ? kDocAtZero : i == n - 1 ? kDocAtEnd : (uint32_t)(i - 1);
        out[i] = k == kDocAtZero ? 0ULL : k == kDocAtEnd ? total : cut_off[k];
    }
}

// ------------------------------------------------------------------ 5''. spans (encode with offsets)
// For every id the half-open byte span, relative to its document, of the merge piece that
// produced it.  The scan's kPos instantiations leave every record's first byte (ScanCutsPos); a
// word's ids tile its bytes in order, so id j of a record starts at the record's position plus
// the byte lengths of ids 0..j-1, and the length of an id is a property of the vocab: a table
// built once per tokenizer (SpanLens).  A special's record takes sp_len instead (its id may be
// shared with an ordinary entry), and a dropped pre-token (info 0) has bytes and no id, so the
// next span starts past it.

// id -> byte length, open addressing: an entry is id << 32 | (length + 1), 0 an empty slot
struct SpanLens {
    const unsigned long long* ent;
    unsigned long long mask;   // slots - 1
};
__host__ __device__ inline size_t span_len_slot(uint32_t id, unsigned long long mask) {
    return (size_t)(mix64((uint64_t)id + 1) & mask);
}
__device__ __forceinline__ uint32_t span_len_of(const SpanLens& L, uint32_t id) {
    size_t sl = span_len_slot(id, L.mask);
    for (;;) {
        const unsigned long long e = L.ent[sl];
        if (e == 0) return 0u;   // no such id: the sum check reports it
        if ((uint32_t)(e >> 32) == id) return (uint32_t)e - 1u;
        sl = (sl + 1) & L.mask;
    }
}

// per chunk: the first byte of the first record after the chunk's own (the end of its last
// record), n when there is none.  A chunk without a record lies inside one pre-token, which is
// under 8 MiB, so the walk is short.
__global__ void k_enc_chunk_next(const uint32_t* __restrict__ rec_n, const unsigned long long* __restrict__ rec_base,
                                 const uint16_t* __restrict__ rec_pos, size_t n_chunks, unsigned long long n,
                                 unsigned long long* __restrict__ next) {
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += (size_t)gridDim.x * blockDim.x) {
        unsigned long long e = n;
        for (size_t d = c + 1; d < n_chunks; ++d)
            if (rec_n[d]) {
                e = (unsigned long long)d * kChunk + rec_pos[rec_base[d]];
                break;
            }
        next[c] = e;
    }
}

struct SpanArgs {
    const uint16_t* rec_pos;             // per record: its first byte, relative to its chunk
    const unsigned long long* next;      // per chunk: k_enc_chunk_next
    const unsigned long long* cuts;      // the document starts inside the text: sorted, distinct
    const uint32_t* chunk_cut0;          // n_chunks + 1: the first cut at or after each chunk's first byte
    const uint32_t* sp_len;
    SpanLens L;
};
constexpr unsigned kSpanStatus = 512u;   // status: a word's id lengths do not sum to its bytes

// one record's spans through put(position, start, end), from position o; returns its ids.
// pos / end: the record's bytes in the text; doc: its document's first byte.
template <class Put>
__device__ __forceinline__ uint32_t put_spans(const EmitArgs& A, const SpanArgs& P, uint32_t rec, unsigned long long info,
                                              unsigned long long pos, unsigned long long end, unsigned long long doc,
                                              uint32_t o, const Put& put) {
    if (info == 0) return 0;
    const uint32_t s0 = (uint32_t)(pos - doc);   // a document is under 2^32 bytes (checked on the host)
    if ((rec & kRecPendBit) && (rec & kRecKind3) == kRecSpecial) {
        const uint32_t l = P.sp_len[rec & kRecPayload29];
        if (pos + l != end) atomicOr(A.status, kSpanStatus);
        put(o, s0, s0 + l);
        return 1;
    }
    uint32_t cur = s0, nm;
    if (info & kInlineIds) {
        uint32_t ids[4];
        nm = info_inline_ids(info, ids);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (j < nm) {
                const uint32_t l = span_len_of(P.L, ids[j]);
                put(o + j, cur, cur + l);
                cur += l;
            }
    } else {
        nm = info_nids(info);
        const uint32_t* src = ((info & kDictPool) ? A.D.pool : A.pool) + (info & kPoolOff);
        for (uint32_t j = 0; j < nm; ++j) {
            const uint32_t l = span_len_of(P.L, src[j]);
            put(o + j, cur, cur + l);
            cur += l;
        }
    }
    if ((unsigned long long)(cur - s0) != end - pos) atomicOr(A.status, kSpanStatus);
    return nm;
}

// The emit's write pass once more, for the spans: the same parts, the same coff and the same three
// paths (LDS-staged, straight to memory when a part has more ids than LDS holds, rounds of 256
// when it has more records than the registers hold).  It runs after the ids' write pass and
// reads the infos that pass read; the ids-only kernels are not touched.  out: uint32_t[2] per id,
// 8-byte aligned; the staged path stores two spans per 16-byte write after a one-span head.
__global__ void __launch_bounds__(256) k_enc_emit_spans(EmitArgs A, SpanArgs P, unsigned long long n, uint2* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint2 buf[kEmitIds];
    __shared__ uint32_t s_ws[4];
    const int tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < A.n_chunks * kEmitParts; c += gridDim.x) {   // c: a part
        const size_t ch = c / kEmitParts;
        const unsigned part = (unsigned)(c % kEmitParts);
        const uint32_t mc = A.rec_n[ch];
        // (the emit's split of the chunk's records into parts)
        const uint32_t r0 = (uint32_t)((unsigned long long)mc * part / kEmitParts),
                       r1 = (uint32_t)((unsigned long long)mc * (part + 1) / kEmitParts);
        const uint32_t m = r1 - r0;
        const uint32_t* __restrict__ r = A.recs + A.rec_base[ch] + r0;
        const uint16_t* __restrict__ rp = P.rec_pos + A.rec_base[ch] + r0;
        const unsigned long long cbase = (unsigned long long)ch * kChunk;
        const unsigned long long cnext = P.next[ch];
        const uint32_t q0 = P.chunk_cut0[ch], q1 = P.chunk_cut0[ch + 1];
        // record i of the part: its first byte, its end, its document's first byte
        auto rec_pos = [&](uint32_t i) -> unsigned long long { return cbase + rp[i]; };
        auto rec_end = [&](uint32_t i) -> unsigned long long { return r0 + i + 1 < mc ? cbase + rp[i + 1] : cnext; };
        auto doc_of = [&](unsigned long long p) -> unsigned long long {
            uint32_t lo = q0, hi = q1;   // the cuts of this chunk that are <= p: [q0, lo)
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (P.cuts[mid] <= p) lo = mid + 1;
                else hi = mid;
            }
            return lo ? P.cuts[lo - 1] : 0ULL;
        };
        if (m <= 256u * kEmitR) {
            const uint32_t R = (m + 255) >> 8;
            const uint32_t lo = tid * R, hi = lo + R < m ? lo + R : m;
            unsigned long long info[kEmitR];
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) info[i] = lo + i < hi ? rec_info(A, r[lo + i]) : 0ULL;
            uint32_t sum = 0;
#pragma unroll
            for (int i = 0; i < kEmitR; ++i) sum += lo + i < hi ? info_nids(info[i]) : 0u;
            uint32_t T;
            const uint32_t toff = block_excl_scan(sum, s_ws, &T);
            const unsigned long long O = A.coff[c];
            if (T <= kEmitIds) {
                uint32_t o = toff;
#pragma unroll
                for (int i = 0; i < kEmitR; ++i)
                    if (lo + i < hi) {
                        const unsigned long long p = rec_pos(lo + i);
                        o += put_spans(A, P, r[lo + i], info[i], p, rec_end(lo + i), doc_of(p), o,
                                       [&](uint32_t q, uint32_t a, uint32_t b) { buf[q] = make_uint2(a, b); });
                    }
                __syncthreads();
                const unsigned h = (((uintptr_t)(out + O) & 15) != 0 && T) ? 1u : 0u;
                if (tid == 0 && h) out[O] = buf[0];
                const unsigned body = (T - h) / 2;
                uint4* dst = reinterpret_cast<uint4*>(out + O + h);
                for (unsigned i = tid; i < body; i += 256) {
                    const uint2 a = buf[h + 2 * i], b = buf[h + 2 * i + 1];
                    dst[i] = make_uint4(a.x, a.y, b.x, b.y);
                }
                if (tid == 0 && h + 2 * body < T) out[O + T - 1] = buf[T - 1];
                __syncthreads();   // buf is reused by the next part
            } else {   // too many ids for LDS: straight to memory
                uint32_t o = toff;
#pragma unroll
                for (int i = 0; i < kEmitR; ++i)
                    if (lo + i < hi) {
                        const unsigned long long p = rec_pos(lo + i);
                        o += put_spans(A, P, r[lo + i], info[i], p, rec_end(lo + i), doc_of(p), o,
                                       [&](uint32_t q, uint32_t a, uint32_t b) { out[O + q] = make_uint2(a, b); });
                    }
            }
        } else {   // many records: rounds of 256
            const unsigned long long O = A.coff[c];
            uint32_t run = 0;
            for (uint32_t b = 0; b < m; b += 256) {
                const bool in = b + tid < m;
                const unsigned long long inf = in ? rec_info(A, r[b + tid]) : 0ULL;
                uint32_t rt;
                const uint32_t off = block_excl_scan(in ? info_nids(inf) : 0u, s_ws, &rt);
                if (in) {
                    const unsigned long long p = rec_pos(b + tid);
                    put_spans(A, P, r[b + tid], inf, p, rec_end(b + tid), doc_of(p), run + off,
                              [&](uint32_t q, uint32_t a, uint32_t bb) { out[O + q] = make_uint2(a, bb); });
                }
                run += rt;
            }
        }
    }
    (void)n;
}

// ---- unit "char": byte spans -> character spans.  C(p) = the bytes of text[0, p) that are not
// continuation bytes (b & 0xC0 != 0x80).  k_char_blocks counts them per 64-byte block of the
// ADDRESS grid (block b = text positions [64 b - lead, 64 b - lead + 64), lead = the text
// pointer's offset in its 64-byte line, so every load is aligned whatever the pointer), one
// exclusive scan gives the blocks' prefix, and k_span_chars maps each span: start -> C(start) -
// (1 if text[start] is a continuation byte), end -> C(end), both less C(document start).

// the non-continuation bytes of a dword, one bit (bit 6) per byte
__device__ __forceinline__ uint32_t noncont4(uint32_t w) {
    const uint32_t x = (w & 0xC0C0C0C0u) ^ 0x80808080u;   // a continuation byte becomes 0
    return (x | (x >> 1)) & 0x40404040u;
}

// a thread takes 16-byte units (aligned loads; a unit that the text only partly covers byte by
// byte); four neighbouring lanes sum to one block
__global__ void __launch_bounds__(256) k_char_blocks(const uint8_t* __restrict__ s, size_t n, size_t n_blocks,
                                                     unsigned long long* __restrict__ cnt) {
    const size_t lead = reinterpret_cast<uintptr_t>(s) & 63;
    const uint8_t* const a0 = s - lead;
    const size_t nv = n_blocks * 4;
    const size_t S = (size_t)gridDim.x * blockDim.x;
    for (size_t v0 = (size_t)blockIdx.x * blockDim.x; v0 < nv; v0 += S) {   // uniform over the workgroup
        const size_t v = v0 + threadIdx.x;
        uint32_t k = 0;
        if (v < nv) {
            const long long p0 = (long long)(16 * v) - (long long)lead;   // text position of byte 0
            if (p0 >= 0 && p0 + 16 <= (long long)n) {
                const uint4 q = *reinterpret_cast<const uint4*>(a0 + 16 * v);
                k = __popc(noncont4(q.x)) + __popc(noncont4(q.y)) + __popc(noncont4(q.z)) + __popc(noncont4(q.w));
            } else {
                for (int j = 0; j < 16; ++j) {
                    const long long p = p0 + j;
                    if (p >= 0 && p < (long long)n) k += (s[p] & 0xC0u) != 0x80u;
                }
            }
        }
        k += __shfl_xor(k, 1);
        k += __shfl_xor(k, 2);
        if (v < nv && (v & 3) == 0) cnt[v >> 2] = k;
    }
}

// C(p) for 0 <= p <= n: the block's prefix plus the non-continuation bytes of the block before p
__device__ __forceinline__ unsigned long long char_index(const uint8_t* __restrict__ s, size_t n, size_t lead,
                                                         const unsigned long long* __restrict__ pre, size_t n_blocks,
                                                         unsigned long long p) {
    const size_t b = (size_t)((p + lead) >> 6);
    if (b >= n_blocks) return pre[n_blocks];   // p == n on a block boundary: the total
    unsigned long long c = pre[b];
    const long long bs = (long long)(b << 6) - (long long)lead;   // text position of the block's byte 0
    // aligned 8-byte words of the block that lie wholly in [0, p); the rest byte by byte
    long long q = bs < 0 ? 0 : bs;
    for (; q < (long long)p && ((q + (long long)lead) & 7); ++q) c += (s[q] & 0xC0u) != 0x80u;
    for (; q + 8 <= (long long)p; q += 8) {
        const uint2 w = *reinterpret_cast<const uint2*>(s + q);
        c += __popc(noncont4(w.x)) + __popc(noncont4(w.y));
    }
    for (; q < (long long)p; ++q) c += (s[q] & 0xC0u) != 0x80u;
    (void)n;
    return c;
}

// one thread per id: its document (the last one whose first id is at or before it), then both ends
__global__ void __launch_bounds__(256) k_span_chars(const uint8_t* __restrict__ s, size_t n,
                                                    const unsigned long long* __restrict__ pre, size_t n_blocks,
                                                    const unsigned long long* __restrict__ id_off,
                                                    const unsigned long long* __restrict__ doc_start, size_t n_docs,
                                                    size_t n_ids, uint2* __restrict__ spans) {
    const size_t lead = reinterpret_cast<uintptr_t>(s) & 63;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ids; i += (size_t)gridDim.x * blockDim.x) {
        size_t lo = 0, hi = n_docs - 1;   // the last document with id_off[d] <= i
        while (lo < hi) {
            const size_t mid = (lo + hi + 1) >> 1;
            if (id_off[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const unsigned long long d0 = doc_start[lo];
        const uint2 sp = spans[i];
        const unsigned long long a = d0 + sp.x, e = d0 + sp.y;
        const unsigned long long cd = char_index(s, n, lead, pre, n_blocks, d0);
        unsigned long long ca = char_index(s, n, lead, pre, n_blocks, a);
        if (a < n && (s[a] & 0xC0u) == 0x80u) --ca;
        const unsigned long long ce = char_index(s, n, lead, pre, n_blocks, e);
        spans[i] = make_uint2((uint32_t)(ca - cd), (uint32_t)(ce - cd));
    }
}

// ------------------------------------------------------------------ 6. padded rows
// CSR ids (u32 ids, u64 row offsets) -> a dense [n_rows, row_len] matrix of OutT (int32 / int64)
// and the rows' kept lengths.  Flags as bpe_ids_pack_rows_device: a row longer than row_len keeps
// its first ids, or with kPackKeepLast its last; a shorter one is padded on the right, or with
// kPackPadLeft on the left.  A thread fills one 16-byte unit of the output (kVec: row_len is a
// multiple of the unit and the matrix is 16-byte aligned, so a unit lies in one row) or one
// element; consecutive threads write consecutive addresses and read consecutive ids.  A kept id
// that an int32 cannot hold (>= 2^31) is reported instead of wrapped: over[0] = 1 and over[1] =
// the smallest such id (over[1] starts at ~0u); the int64 rows hold every id.
constexpr int kPackKeepLast = 1, kPackPadLeft = 2;

template <class OutT, bool kVec>
__global__ void __launch_bounds__(256) k_pack_rows(const uint32_t* __restrict__ ids, const unsigned long long* __restrict__ off,
                                                   size_t n_rows, size_t row_len, OutT pad, int flags,
                                                   OutT* __restrict__ out, int32_t* __restrict__ lengths,
                                                   unsigned* __restrict__ over) {
    constexpr unsigned kPer = kVec ? 16 / sizeof(OutT) : 1;
    constexpr bool kNarrow = sizeof(OutT) == 4;
    uint32_t worst = 0xffffffffu;   // this thread's smallest id >= 2^31
    bool wide = false;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = t0; i < n_rows; i += stride) {
        const unsigned long long L = off[i + 1] - off[i];
        lengths[i] = (int32_t)(L < row_len ? L : row_len);
    }
    const size_t units = n_rows * row_len / kPer;
    for (size_t u = t0; u < units; u += stride) {
        const size_t e = u * kPer, row = e / row_len, col = e - row * row_len;
        const unsigned long long a = off[row], L = off[row + 1] - a;
        const size_t len = L < row_len ? (size_t)L : row_len;
        const unsigned long long src = (flags & kPackKeepLast) ? a + L - len : a;   // the first id kept
        const size_t c0 = (flags & kPackPadLeft) ? row_len - len : 0;               // its column
        OutT v[kPer];
#pragma unroll
        for (unsigned k = 0; k < kPer; ++k) {
            const size_t cc = col + k;
            const bool kept = cc >= c0 && cc < c0 + len;
            const uint32_t id = kept ? ids[src + (cc - c0)] : 0u;
            if (kNarrow && id >= 0x80000000u) {
                wide = true;
                worst = id < worst ? id : worst;
            }
            v[k] = kept ? (OutT)id : pad;
        }
        if (kVec) {
            uint4 w;
            __builtin_memcpy(&w, v, 16);
            *reinterpret_cast<uint4*>(out + e) = w;
        } else {
            out[e] = v[0];
        }
    }
    if (kNarrow && __ballot(wide)) {   // (every thread of the wave is here: no early return above)
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t w = __shfl_xor(worst, o);
            worst = w < worst ? w : worst;
        }
        if ((threadIdx.x & 63) == 0) {
            atomicOr(&over[0], 1u);
            atomicMin(&over[1], worst);
        }
    }
}

__device__ __forceinline__ uint2 rank_of(const EncTables& E, uint32_t a, uint32_t b) {
    const unsigned long long key = ((((unsigned long long)a) << 32) | b) + 1ULL;
    size_t s = mix64(key) & E.pm_mask;
    for (;;) {
        const unsigned long long k = E.pm_key[s];
        if (k == key) return E.pm_val[s];
        if (k == 0) return make_uint2(0xffffffffu, 0);
        s = (s + 1) & E.pm_mask;
    }
}

// tokenizer.py:124-136 for one unique word; the ids are written once into the word's slot
__global__ void __launch_bounds__(256)
k_encode_words(const uint8_t* __restrict__ s, EncTables E, const unsigned long long* __restrict__ w_off,
               const uint32_t* __restrict__ w_len, const unsigned long long* __restrict__ w_idoff,
               const uint32_t* __restrict__ w_slot, unsigned n_words, uint32_t* __restrict__ pool,
               unsigned long long* __restrict__ slot_info, unsigned* __restrict__ status, size_t n) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t len = w_len[w];
    unsigned long long* info = slot_info + w_slot[w];
    if (w_off[w] + len > n) { atomicOr(status, 64u); *info = 0; return; }   // a bug: report
    const uint8_t* src = s + w_off[w];
    for (int k = 0; k < E.n_sp; ++k)  // match() drops pre-tokens equal to a special (73)
        if (E.sp_len[k] == len && bytes_eq(src, E.sp_bytes + E.sp_off[k], len)) { *info = 0; return; }
    uint32_t* t = pool + w_idoff[w];
    for (uint32_t i = 0; i < len; ++i) t[i] = E.byte2tok[src[i]];
    uint32_t m = len;
    while (m > 1) {
        uint32_t best = 0xffffffffu, prod = 0, ba = 0, bb = 0;
        for (uint32_t i = 0; i + 1 < m; ++i) {
            const uint2 r = rank_of(E, t[i], t[i + 1]);
            if (r.x < best) { best = r.x; prod = r.y; ba = t[i]; bb = t[i + 1]; }
        }
        if (best == 0xffffffffu) break;
        uint32_t j = 0;  // merge() (92-109): every occurrence, left to right
        for (uint32_t i = 0; i < m;) {
            if (t[i] == ba && i + 1 < m && t[i + 1] == bb) { t[j++] = prod; i += 2; }
            else t[j++] = t[i++];
        }
        m = j;
    }
    for (uint32_t i = 0; i < m; ++i) {
        const int64_t v = E.tok2vid[t[i]];
        if (v < 0) atomicOr(status, 4u);
        t[i] = (uint32_t)v;
    }
    *info = make_info(m, t, w_idoff[w]);
}

__global__ void k_word_len64(const uint32_t* __restrict__ w_len, unsigned n, unsigned long long* __restrict__ o) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = w_len[i];
}

}  // namespace
}  // namespace bpe

// =================================================================== the tokenizer object
struct bpe_tokenizer {
    std::vector<std::string> specials;     // deduped, longest first
    std::vector<int64_t> special_vid;
    hipStream_t stream = nullptr;
    bpe::DevBuf<unsigned long long> pm_key;
    bpe::DevBuf<uint2> pm_val;
    size_t pm_cap = 0;
    bpe::DevBuf<int64_t> tok2vid;
    bpe::DevBuf<uint32_t> byte2tok;
    bpe::DevBuf<uint8_t> sp_bytes;
    bpe::DevBuf<uint32_t> sp_off, sp_len;
    bpe::DevBuf<int64_t> sp_vid;
    bpe::DevBuf<unsigned> first_mask;
    // the encoder's dictionary (build_dictionary): every vocab entry of 2..16 bytes with its ids,
    // the one-byte words' records
    bpe::DevBuf<bpe::DictEnt> dict_ent;
    bpe::DevBuf<uint32_t> dict_pool, byte_rec, dict_filt;
    size_t dict_slots = 0, dict_words = 0;
    // the span calls' id -> byte length table (bpe::SpanLens); span_shared: some id names byte
    // strings of different lengths, so the span calls are refused (decided once, at creation)
    bpe::DevBuf<unsigned long long> span_len;
    size_t span_slots = 0;
    bool span_shared = false;
    // the per-pre-token record buffer, kept for the next call: freeing and re-allocating tens of
    // GB per call costs up to seconds in the driver (measured 0.5 -> 2.8 s for an 11.9 GB
    // encode).  Calls on one handle are serialized on its stream.
    bpe::DevBuf<uint32_t> recs_cache;
    // the other per-call device arrays, kept the same way (grow-only): per chunk, per word-table
    // slot, per unique word, the id pool, the u16 output of the bulk encoder
    struct Scratch {
        bpe::DevBuf<uint32_t> rec_n, w_slot, w_len, pool, block_used;
        bpe::DevBuf<unsigned long long> rec_base, rec_fill, fill, kv, pos, w_off, len64, idoff, slot_info;
        bpe::DevBuf<unsigned> status, d_nw, pend_nblk;
        bpe::DevBuf<unsigned long long> ctot, coff;   // per chunk: ids, first id's position
        bpe::DevBuf<unsigned long long> rstats;       // the resolve's counters (BPE355_TRACE)
        bpe::PieceScratch piece;                      // encode_file's piece-start search
        bpe::DevBuf<unsigned long long> pend;   // the scan's pending entries (resolved in place)
        bpe::DevBuf<bpe::Seg> segs;
        bpe::DevBuf<unsigned long long> sp_key, sp_sorted;   // special matches, (position << 16 | index)
        bpe::DevBuf<unsigned long long> sp_cnt, sp_off, cuts;   // the device segment builder's arrays
        bpe::DevBuf<uint8_t> sp_flag;
        bpe::DevBuf<uint8_t> tmp;
        bpe::DevBuf<uint16_t> ids16;
        bpe::DevBuf<uint8_t> text, text2;   // the bulk encoder's file bytes (and its newline-translated copy)
        // encode_batch: per chunk its first cut, per cut its record index and id offset, per document its cut
        bpe::DevBuf<uint32_t> chunk_cut0, cut_rec, doc_cut;
        bpe::DevBuf<unsigned long long> cut_off;
        // the span calls: per record its position, per chunk the end of its last record, the
        // character counts of the text's 64-byte blocks and their prefix, the document starts
        bpe::DevBuf<uint16_t> rec_pos;
        bpe::DevBuf<unsigned long long> chunk_next, char_cnt, char_pre, doc_start;
        bpe::DropScratch drop;   // encode with dropout (dropout.hip)
        // the dataset encoder (encode_files_pipelined): the raw read ring, the translated text and
        // the buffer its carry moves through, the id ring, one region's separator positions, the
        // id table
        struct Dataset {
            bpe::DevBuf<uint8_t> raw[2], text, move, ids[2];
            bpe::DevBuf<unsigned long long> pos, counts;
            bpe::IdScratch stat;
        } ds;
    } sc;
    // construction inputs, to build the same tables for the other ranks of a multi-device encode
    // (bpe_tok_encode_gpus); those copies own their stream and record buffer
    std::string vblob, mblob;
    std::vector<std::string> sp_in;
    int device = 0;
    // ill-formed UTF-8 in bpe_tok_encode_files (bpe_tok_set_errors): the mode, and what the last
    // call repaired (the totals, the file of the first span, the spans per file)
    int errors = 0;
    bpe_utf8_stats fix_total{0, 0, ~0ULL};
    uint64_t fix_first_file = 0;
    std::vector<uint64_t> fix_file_units;
    std::mutex copies_m;
    std::vector<std::pair<long long, std::unique_ptr<bpe_tokenizer>>> copies;   // (rank << 8 | device)
    ~bpe_tokenizer() {
        if (stream) (void)hipStreamDestroy(stream);
    }
    bpe::EncTables tables() const {
        return bpe::EncTables{pm_key.p, pm_val.p, (unsigned long long)(pm_cap - 1), tok2vid.p,
                              byte2tok.p, sp_bytes.p, sp_off.p, sp_len.p, sp_vid.p,
                              (int)specials.size()};
    }
    bpe::SpanLens span_lens() const { return bpe::SpanLens{span_len.p, (unsigned long long)(span_slots - 1)}; }
    bpe::EncDict dict() const {
        return bpe::EncDict{dict_ent.p, (unsigned long long)(dict_slots - 1), dict_pool.p, byte_rec.p, dict_filt.p};
    }
};

namespace bpe {
namespace {

uint32_t rd_u32(const uint8_t*& p, const uint8_t* end) {
    BPE_REQUIRE(p + 4 <= end, BPE_E_ARG, "truncated blob");
    uint32_t v;
    std::memcpy(&v, p, 4);
    p += 4;
    return v;
}

// The encoder's dictionary: every vocab entry of 2..16 bytes, encoded once on the device by
// k_encode_words exactly as a pre-token of those bytes is (tokenizer.py:124-136), in an open-
// addressing table keyed by the packed bytes; plus the record of every one-byte word.  Entries
// whose encoding has an id outside the direct range (or a missing vocab id: the KeyError path)
// are left out, so those words take the word table as before.
void build_dictionary(bpe_tokenizer& T, const std::unordered_map<std::string, uint32_t>& intern,
                      const std::vector<int64_t>& vid, const std::vector<uint32_t>& b2t) {
    std::vector<const std::string*> cand;
    for (const auto& kv : intern)
        if (kv.first.size() >= 2 && kv.first.size() <= (size_t)kInline && vid[kv.second] >= 0)
            cand.push_back(&kv.first);
    std::sort(cand.begin(), cand.end(), [](const std::string* a, const std::string* b) { return *a < *b; });
    const size_t nc = cand.size();
    std::vector<unsigned long long> info(nc);
    std::vector<uint32_t> pool;
    if (nc) {
        std::string text;
        std::vector<unsigned long long> off(nc), idoff(nc);
        std::vector<uint32_t> len(nc), slot(nc);
        for (size_t i = 0; i < nc; ++i) {
            off[i] = text.size();
            idoff[i] = text.size();   // ids <= bytes: the pool mirrors the text
            len[i] = (uint32_t)cand[i]->size();
            slot[i] = (uint32_t)i;
            text += *cand[i];
        }
        DevBuf<uint8_t> d_text(text.size());
        DevBuf<unsigned long long> d_off(nc), d_idoff(nc), d_info(nc);
        DevBuf<uint32_t> d_len(nc), d_slot(nc), d_pool(text.size());
        DevBuf<unsigned> d_status(1);
        to_device(d_text.p, text.data(), text.size(), T.stream);
        to_device(d_off.p, off.data(), nc * 8, T.stream);
        to_device(d_idoff.p, idoff.data(), nc * 8, T.stream);
        to_device(d_len.p, len.data(), nc * 4, T.stream);
        to_device(d_slot.p, slot.data(), nc * 4, T.stream);
        BPE_HIP(hipMemsetAsync(d_status.p, 0, 4, T.stream));
        hipLaunchKernelGGL(k_encode_words, dim3(ceil_div(nc, 256)), dim3(256), 0, T.stream, d_text.p, T.tables(),
                           d_off.p, d_len.p, d_idoff.p, d_slot.p, (unsigned)nc, d_pool.p, d_info.p, d_status.p,
                           text.size());
        BPE_HIP(hipGetLastError());
        pool.resize(text.size());
        to_host(info.data(), d_info.p, nc * 8, T.stream);
        to_host(pool.data(), d_pool.p, text.size() * 4, T.stream);
    }
    T.dict_slots = next_pow2(std::max<size_t>(64, 2 * nc));
    std::vector<DictEnt> ent(T.dict_slots);
    std::memset(ent.data(), 0, ent.size() * sizeof(DictEnt));
    std::vector<uint32_t> dpool;
    size_t words = 0;
    for (size_t i = 0; i < nc; ++i) {
        const unsigned long long inf = info[i];
        std::vector<uint32_t> ids;
        if (inf & kInlineIds) {
            uint32_t x[4];
            ids.assign(x, x + info_inline_ids(inf, x));
        } else if (inf) {
            const uint32_t nm = info_nids(inf);
            const size_t o = (size_t)(inf & kPoolOff);
            ids.assign(pool.begin() + o, pool.begin() + o + nm);
        }
        bool ok = true;
        for (uint32_t x : ids) ok = ok && x < kRecPayload;
        if (!ok) continue;
        const std::string& w = *cand[i];
        uint64_t lo = 0, hi = 0;
        for (size_t j = 0; j < w.size(); ++j) {
            const uint64_t b = (uint8_t)w[j];
            if (j < 8) lo |= b << (8 * j);
            else hi |= b << (8 * (j - 8));
        }
        size_t sl = short_hash(lo, hi, w.size()) & (T.dict_slots - 1);
        while (ent[sl].len) sl = (sl + 1) & (T.dict_slots - 1);
        DictEnt& e = ent[sl];
        e.lo = lo;
        e.hi = hi;
        e.len = (uint32_t)w.size();
        if (ids.size() == 1) {
            e.rec = kRecDirect | ids[0];
            e.info = kOneId | ids[0];
        } else {
            e.rec = kDictMark | (uint32_t)sl;
            e.info = make_info((uint32_t)ids.size(), ids.data(), kDictPool | dpool.size());
            if (!ids.empty() && !(e.info & kInlineIds)) dpool.insert(dpool.end(), ids.begin(), ids.end());
        }
        ++words;
    }
    T.dict_words = words;
    std::vector<uint32_t> brec(256, kRecNone);
    for (int b = 0; b < 256; ++b) {
        const int64_t v = vid[b2t[b]];
        bool special = false;
        for (const auto& sp : T.specials) special = special || (sp.size() == 1 && (uint8_t)sp[0] == b);
        if (v >= 0 && v < (int64_t)kRecPayload && !special) brec[b] = kRecDirect | (uint32_t)v;
    }
    T.dict_ent.alloc(ent.size());
    to_device(T.dict_ent.p, ent.data(), ent.size() * sizeof(DictEnt), T.stream);
    T.dict_pool.alloc(std::max<size_t>(dpool.size(), 1));
    if (!dpool.empty()) to_device(T.dict_pool.p, dpool.data(), dpool.size() * 4, T.stream);
    T.byte_rec.alloc(256);
    to_device(T.byte_rec.p, brec.data(), 256 * 4, T.stream);
    std::vector<uint32_t> filt(kFiltBits / 32, 0u);
    for (const DictEnt& e : ent)
        if (e.len) {
            const unsigned i = filt_index(short_hash(e.lo, e.hi, e.len));
            filt[i >> 5] |= 1u << (i & 31);
        }
    T.dict_filt.alloc(filt.size());
    to_device(T.dict_filt.p, filt.data(), filt.size() * 4, T.stream);
    BPE_HIP(hipStreamSynchronize(T.stream));
}

void build_tokenizer(bpe_tokenizer& T, const uint8_t* vb, size_t vn, const uint8_t* mb, size_t mn,
                     const std::vector<std::string>& sp_in) {
    std::unordered_map<std::string, uint32_t> intern;
    std::vector<int64_t> vid;
    auto tok = [&](const std::string& s) {
        auto it = intern.find(s);
        if (it != intern.end()) return it->second;
        const uint32_t id = (uint32_t)intern.size();
        intern.emplace(s, id);
        vid.push_back(-1);
        return id;
    };
    // vocab_inv = {bytes: id}: last id wins (tokenizer.py:19)
    const uint8_t* p = vb;
    const uint8_t* end = vb + vn;
    const uint32_t nv = rd_u32(p, end);
    for (uint32_t i = 0; i < nv; ++i) {
        BPE_REQUIRE(p + 12 <= end, BPE_E_ARG, "truncated vocab blob");
        int64_t id;
        std::memcpy(&id, p, 8);
        p += 8;
        const uint32_t l = rd_u32(p, end);
        BPE_REQUIRE(p + l <= end, BPE_E_ARG, "truncated vocab blob");
        BPE_REQUIRE(id >= 0 && id < (1LL << 32), BPE_E_ARG, "vocab id outside [0, 2^32)");
        vid[tok(std::string((const char*)p, l))] = id;
        p += l;
    }
    // specials: dedupe (first occurrence), longest first; missing ones get ids len(vocab), ...
    std::unordered_set<std::string> seen_sp;   // (a linear search per special: seconds at the 65 535 limit)
    for (const auto& s : sp_in) {
        BPE_REQUIRE(!s.empty(), BPE_E_ARG, "empty special token is not supported");
        if (seen_sp.insert(s).second) T.specials.push_back(s);
    }
    std::stable_sort(T.specials.begin(), T.specials.end(),
                     [](const std::string& x, const std::string& y) { return x.size() > y.size(); });
    int64_t next_id = (int64_t)nv;
    for (const auto& s : T.specials) {
        const uint32_t t = tok(s);
        if (vid[t] < 0) vid[t] = next_id++;
        T.special_vid.push_back(vid[t]);
    }
    // merges: rank = index, later duplicates overwrite (tokenizer.py:115)
    std::unordered_map<unsigned long long, std::pair<uint32_t, uint32_t>> rank;
    p = mb;
    end = mb + mn;
    const uint32_t nm = rd_u32(p, end);
    for (uint32_t i = 0; i < nm; ++i) {
        const uint32_t la = rd_u32(p, end);
        BPE_REQUIRE(p + la <= end, BPE_E_ARG, "truncated merges blob");
        std::string a((const char*)p, la);
        p += la;
        const uint32_t lb = rd_u32(p, end);
        BPE_REQUIRE(p + lb <= end, BPE_E_ARG, "truncated merges blob");
        std::string b((const char*)p, lb);
        p += lb;
        const uint32_t ta = tok(a), tb = tok(b), tp = tok(a + b);
        rank[((unsigned long long)ta << 32) | tb] = {i, tp};
    }
    std::vector<uint32_t> b2t(256);
    for (int b = 0; b < 256; ++b) b2t[b] = tok(std::string(1, (char)b));

    // device tables
    T.pm_cap = next_pow2(std::max<size_t>(64, rank.size() * 2 + 1));
    std::vector<unsigned long long> hk(T.pm_cap, 0);
    std::vector<uint2> hv(T.pm_cap);
    for (const auto& kv : rank) {
        const unsigned long long key = kv.first + 1ULL;
        size_t s = mix64(key) & (T.pm_cap - 1);
        while (hk[s]) s = (s + 1) & (T.pm_cap - 1);
        hk[s] = key;
        hv[s] = make_uint2(kv.second.first, kv.second.second);
    }
    BPE_HIP(hipStreamCreateWithFlags(&T.stream, hipStreamNonBlocking));
    auto up = [&](auto& buf, const auto& vec) {
        buf.alloc(std::max<size_t>(vec.size(), 1));
        if (!vec.empty())
            BPE_HIP(hipMemcpyAsync(buf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, T.stream));
    };
    up(T.pm_key, hk);
    up(T.pm_val, hv);
    up(T.tok2vid, vid);
    up(T.byte2tok, b2t);
    std::string spb;
    std::vector<uint32_t> spo, spl;
    std::vector<unsigned> fm(8, 0);
    for (const auto& s : T.specials) {
        spo.push_back((uint32_t)spb.size());
        spl.push_back((uint32_t)s.size());
        spb += s;
        const unsigned char c = (unsigned char)s[0];
        fm[c >> 5] |= 1u << (c & 31);
    }
    std::vector<uint8_t> spbv(spb.begin(), spb.end());
    up(T.sp_bytes, spbv);
    up(T.sp_off, spo);
    up(T.sp_len, spl);
    up(T.sp_vid, T.special_vid);
    up(T.first_mask, fm);
    BPE_HIP(hipStreamSynchronize(T.stream));
    build_dictionary(T, intern, vid, b2t);
    // the span calls' table: the byte length of every id the encoder can emit
    size_t n_ids = 0;
    for (const int64_t v : vid) n_ids += v >= 0;
    T.span_slots = next_pow2(std::max<size_t>(64, 2 * n_ids));
    std::vector<unsigned long long> sl(T.span_slots, 0ULL);
    for (const auto& kv : intern) {
        const int64_t v = vid[kv.second];
        if (v < 0) continue;
        const uint32_t id = (uint32_t)v;
        const unsigned long long e = ((unsigned long long)id << 32) | (unsigned long long)(kv.first.size() + 1);
        size_t q = span_len_slot(id, T.span_slots - 1);
        while (sl[q] && (uint32_t)(sl[q] >> 32) != id) q = (q + 1) & (T.span_slots - 1);
        if (sl[q] && sl[q] != e) T.span_shared = true;
        sl[q] = e;
    }
    up(T.span_len, sl);
    BPE_HIP(hipStreamSynchronize(T.stream));
}

// encode d_text[0..n) into d_out; returns the id count.  `cuts` (sorted byte offsets) make the
// result that of separate encode() calls on the pieces between them, concatenated: a cut ends
// every segment, and a special token may not straddle one (encode.py's 1 M-character chunks,
// encode_iterable's 2 MiB batches).
// `docs` (encode_batch; its starts are then the cuts): d_out of it gets the id offset of every
// document start and, as entry n_docs, the id count.
struct DocStarts {
    const uint64_t* starts;        // host: non-decreasing, starts[0] == 0, <= n
    size_t n_docs;
    unsigned long long* d_out;     // device: n_docs + 1 entries
};
// `spans` (the span calls; with docs): d_spans gets every id's (start, end) in its document, in
// bytes (unit 0) or characters (unit 1)
struct SpanOut {
    uint2* d_spans;                // device: one per id, 8-byte aligned
    int unit;
};

template <class OutT>
size_t encode_device(bpe_tokenizer& T, const uint8_t* d_text, size_t n, OutT* d_out,
                     hipStream_t s, const std::vector<unsigned long long>& cuts_in = {},
                     const DocStarts* docs = nullptr, const SpanOut* spans = nullptr, const DropParams* drop = nullptr) {
    if (n == 0) return 0;
    std::vector<unsigned long long> cuts;
    for (unsigned long long c : cuts_in)
        if (c > 0 && c < n && (cuts.empty() || c > cuts.back())) cuts.push_back(c);
    // the scan exports the records' positions (with the cuts, if any): the span calls and encode with dropout
    const bool want_pos = docs && (spans || drop);
    const bool want_cuts = docs && (!cuts.empty() || want_pos);   // (no cut: every start is at byte 0 or at the end)
    if (docs) BPE_REQUIRE(cuts.size() < 0xFFFFFFF0ull, BPE_E_LIMIT, "too many documents for one encode");
    bool cuts_up = false;   // S.cuts holds the cuts
    EncTables E = T.tables();
    // 1. segments: every special match (k_find_specials), sorted on the device by (position,
    // index) -- by position, longest first (T.specials is longest first) -- then built into the
    // segment table on the device (k_sp_*), or left to right here when matches overlap
    auto& S = T.sc;
    DevBuf<Seg>& d_segs = S.segs;
    int nseg = 0;
    bool on_device = false;
    std::vector<unsigned long long> keys;
    if (!T.specials.empty()) {
        BPE_REQUIRE(T.specials.size() < (1u << kSpShift) && (n >> (64 - kSpShift)) == 0, BPE_E_LIMIT,
                    "too many special tokens or too long a text");
        unsigned long long cap = std::max<unsigned long long>(1024, n / 64);
        S.status.reserve(1);
        unsigned cnt32 = 0;
        for (;;) {
            S.sp_key.reserve(cap);
            BPE_HIP(hipMemsetAsync(S.status.p, 0, 4, s));
            hipLaunchKernelGGL(k_find_specials, dim3(std::min<unsigned>(grid_for((n + 15) / 16 + 1, 256), 4096)), dim3(256), 0, s, d_text, n, E,
                               T.first_mask.p, S.sp_key.p, S.status.p, cap);
            BPE_HIP(hipGetLastError());
            to_host(&cnt32, S.status.p, 4, s);
            if (cnt32 <= cap) break;
            cap = cnt32;
        }
        if (cnt32) {
            S.sp_sorted.reserve(cnt32);
            unsigned bits = kSpShift;
            while (bits < 64 && (n >> (bits - kSpShift)) != 0) ++bits;
            radix_sort_keys(S.sp_key.p, S.sp_sorted.p, cnt32, bits, s, &S.tmp);
            const size_t nc = cuts.size();
            S.cuts.reserve(std::max<size_t>(nc, 1));
            if (nc) to_device(S.cuts.p, cuts.data(), nc * 8, s);
            cuts_up = true;
            // the matches no cut splits, in order (into sp_key)
            S.sp_flag.reserve(cnt32);
            S.sp_off.reserve(2);
            hipLaunchKernelGGL(k_sp_eligible, dim3(grid_for(cnt32, 256)), dim3(256), 0, s, S.sp_sorted.p,
                               (size_t)cnt32, E.sp_len, S.cuts.p, nc, S.sp_flag.p);
            select_flagged(S.sp_sorted.p, S.sp_flag.p, S.sp_key.p, S.sp_off.p, cnt32, s);
            unsigned long long me = 0;
            to_host(&me, S.sp_off.p, 8, s);
            // segments per kept special (and the tail), their offsets, overlap check
            S.sp_cnt.reserve(me + 1);
            S.sp_off.reserve(me + 1);
            BPE_HIP(hipMemsetAsync(S.status.p, 0, 4, s));
            hipLaunchKernelGGL(k_sp_count, dim3(grid_for(me + 1, 256)), dim3(256), 0, s, S.sp_key.p, (size_t)me,
                               E.sp_len, S.cuts.p, nc, (unsigned long long)n, S.sp_cnt.p, S.status.p);
            exclusive_sum(S.sp_cnt.p, S.sp_off.p, (size_t)me + 1, s, &S.tmp);
            unsigned conflict = 0;
            unsigned long long last[2];
            to_host(&conflict, S.status.p, 4, s);
            to_host(&last[0], S.sp_off.p + me, 8, s);
            to_host(&last[1], S.sp_cnt.p + me, 8, s);
            if (!conflict) {
                const unsigned long long total = last[0] + last[1];
                BPE_REQUIRE(total < (1ull << 31), BPE_E_LIMIT, "too many segments (special tokens and pieces)");
                nseg = (int)total;
                d_segs.reserve(std::max(nseg, 1));
                hipLaunchKernelGGL(k_sp_emit, dim3(grid_for(me + 1, 256)), dim3(256), 0, s, S.sp_key.p, (size_t)me,
                                   E.sp_len, S.cuts.p, nc, (unsigned long long)n, S.sp_off.p, d_segs.p);
                BPE_HIP(hipGetLastError());
                on_device = true;
            } else {
                keys.resize(cnt32);
                to_host(keys.data(), S.sp_sorted.p, (size_t)cnt32 * 8, s);
            }
        }
    }
    if (!on_device) {   // leftmost, non-overlapping (re.split), cut by the pieces
        std::vector<Seg> segs;
        unsigned long long cur = 0;
        size_t ci = 0;
        auto cut_until = [&](unsigned long long upto) {   // normal segments ended by cuts <= upto
            for (; ci < cuts.size() && cuts[ci] <= upto; ++ci) {
                if (cuts[ci] > cur) segs.push_back(Seg{cur, cuts[ci], -1, 0});
                cur = std::max(cur, cuts[ci]);
            }
        };
        for (const unsigned long long key : keys) {
            const unsigned long long p0 = key >> kSpShift;
            const int sk = (int)(key & ((1u << kSpShift) - 1));
            if (p0 < cur) continue;
            const unsigned long long e = p0 + T.specials[sk].size();
            cut_until(p0);
            if (ci < cuts.size() && cuts[ci] < e) continue;   // straddles a cut: a shorter one at p0 may fit
            if (p0 > cur) segs.push_back(Seg{cur, p0, -1, 0});
            segs.push_back(Seg{p0, e, sk, 0});
            cur = e;
        }
        cut_until(n);
        if (cur < n) segs.push_back(Seg{cur, n, -1, 0});
        BPE_REQUIRE(segs.size() < (1ull << 31), BPE_E_LIMIT, "too many segments (special tokens and pieces)");
        nseg = (int)segs.size();
        d_segs.reserve(std::max(nseg, 1));
        to_device(d_segs.p, segs.data(), nseg * sizeof(Seg), s);
    }

    // 2. one staged pass: unique pre-tokens into the word table, one record per pre-token, each
    // chunk's records one dense run
    const size_t n_chunks = (n + kChunk - 1) / kChunk;
    BPE_REQUIRE(n_chunks < (1ull << 32), BPE_E_LIMIT, "text too long for one encode");
    const bool aligned = (reinterpret_cast<uintptr_t>(d_text) & 15u) == 0;
    auto kern = want_cuts ? (aligned ? k_enc_scan4<true, true> : k_enc_scan4<false, true>)
                          : (aligned ? k_enc_scan4<true, false> : k_enc_scan4<false, false>);
    auto kern_pos = aligned ? k_enc_scan4<true, true, true> : k_enc_scan4<false, true, true>;
    int per_cu = 0, dev = 0, n_cu = 0;
    if (want_pos) BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern_pos, 256, kStage));
    else BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, kStage));
    BPE_HIP(hipGetDevice(&dev));
    BPE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    unsigned sgrid = (unsigned)std::min<size_t>(n_chunks, (size_t)std::max(1, per_cu) * std::max(1, n_cu));
    if (const char* e = std::getenv("BPE355_STREAM_WG"))   // test knob (see count_words)
        sgrid = std::max(1u, std::min(sgrid, (unsigned)std::atoi(e)));
    // first guesses: small texts have many more unique words per byte than large corpora; natural
    // text has ~0.15 pre-tokens per byte (at most one per byte: the retry's size)
    // word table: distinct words grow sublinearly with the text (~1.3 M in 64 MB and ~7.5 M in
    // 11.9 GB of the OWT-like bench corpus, about n^0.35); 2.5 x that estimate keeps the load under
    // ~0.4, and a table that fills past 1/2 anyway stops the resolve and is retried 4 x larger
    const double est = 1.32e6 * std::pow(std::max(1.0, (double)n / (double)(1u << 26)), 0.35);
    size_t cap = next_pow2(std::max<size_t>(1 << 16, n < (1u << 26) ? n / 16 : (size_t)(2.5 * est)));
    if (const char* e = std::getenv("BPE355_ENC_TABLE_SLOTS"))   // A/B knob: the first table's slots
        cap = next_pow2(std::max<size_t>(1 << 16, std::strtoull(e, nullptr, 10)));
    unsigned long long rec_cap = n < (1u << 26) ? n + 64 : n / 4 + (1u << 20);
    // records are reserved a region per workgroup at a time: a region holds any chunk, and the
    // regions left part-used (the last of every workgroup, a chunk-sized tail of the others) are
    // slack the buffer carries
    const unsigned long long rec_region =
        std::min<unsigned long long>(1u << 18, std::max<unsigned long long>(kChunk, next_pow2(rec_cap / sgrid / 8)));
    const unsigned long long rec_slack = (unsigned long long)sgrid * rec_region;
    rec_cap += rec_slack + rec_cap / rec_region * kChunk;
    if (const char* e = std::getenv("BPE355_ENC_REC_CAP"))   // test knob: force the record retry
        rec_cap = std::max<unsigned long long>(1, std::strtoull(e, nullptr, 10));
    const unsigned long long rec_cap_max = n + n / 8 + rec_slack + 64;   // one record per byte
    // pending entries: ~0.07 per byte at the bench corpus (the LDS cache's misses); a block per
    // workgroup at least twice over; when the pool is spent the scan resolves words itself
    unsigned long long pend_cap = std::max<unsigned long long>(n / 8, 2ull * sgrid * kPendBlock);
    if (const char* e = std::getenv("BPE355_ENC_PEND_CAP"))   // test knob: a small pool (0: none)
        pend_cap = std::strtoull(e, nullptr, 10);
    pend_cap = std::min<unsigned long long>(pend_cap, (unsigned long long)kRecPendMax + 1 - kPendBlock);
    const unsigned pend_blocks = (unsigned)(pend_cap / kPendBlock);
    DevBuf<unsigned long long>&kv = S.kv, &pos = S.pos;
    DevBuf<unsigned long long>&rec_base = S.rec_base, &rec_fill = S.rec_fill, &fill = S.fill;
    DevBuf<uint32_t>& rec_n = S.rec_n;
    DevBuf<unsigned>& status = S.status;
    rec_base.reserve(n_chunks);
    rec_n.reserve(n_chunks);
    rec_fill.reserve(1);
    fill.reserve(1);
    status.reserve(1);
    S.pend.reserve(std::max<unsigned long long>((unsigned long long)pend_blocks * kPendBlock, 1));
    S.block_used.reserve(std::max(pend_blocks, 1u));
    S.pend_nblk.reserve(1);
    const EncDict D = T.dict();
    ScanCuts SC{nullptr, nullptr, nullptr};
    if (want_cuts) {   // the cuts on the device, and every chunk's first one
        const size_t nc = cuts.size();
        if (!cuts_up) {
            S.cuts.reserve(std::max<size_t>(nc, 1));
            if (nc) to_device(S.cuts.p, cuts.data(), nc * 8, s);
        }
        std::vector<uint32_t> first(n_chunks + 1);
        size_t j = 0;
        for (size_t c = 0; c <= n_chunks; ++c) {
            while (j < nc && cuts[j] < (unsigned long long)c * kChunk) ++j;
            first[c] = (uint32_t)j;
        }
        S.chunk_cut0.reserve(n_chunks + 1);
        to_device(S.chunk_cut0.p, first.data(), (n_chunks + 1) * 4, s);
        S.cut_rec.reserve(std::max<size_t>(nc, 1));
        S.cut_off.reserve(std::max<size_t>(nc, 1));
        SC = ScanCuts{S.cuts.p, S.chunk_cut0.p, S.cut_rec.p};
    }
    const bool tracing = std::getenv("BPE355_TRACE") != nullptr;
    if (tracing) S.rstats.reserve(3);
    unsigned long long pend_entries = 0;   // blocks handed out x kPendBlock (the last attempt's)
    BPE_REQUIRE(T.dict_slots < kRecPayload29 / 2, BPE_E_LIMIT, "vocab too large for the encoder's dictionary");
    for (int attempt = 0;; ++attempt) {
        BPE_REQUIRE(cap + T.dict_slots <= (size_t)kRecPayload29, BPE_E_LIMIT, "too many distinct words for one encode");
        kv.reserve(2 * cap);
        pos.reserve(cap);
        T.recs_cache.reserve(rec_cap);
        if (want_pos) S.rec_pos.reserve(rec_cap);   // (every attempt rewrites it: the kept attempt's stays)
        BPE_HIP(hipMemsetAsync(kv.p, 0, 2 * cap * sizeof(unsigned long long), s));
        BPE_HIP(hipMemsetAsync(status.p, 0, 4, s));
        BPE_HIP(hipMemsetAsync(fill.p, 0, 8, s));
        BPE_HIP(hipMemsetAsync(rec_fill.p, 0, 8, s));
        BPE_HIP(hipMemsetAsync(S.pend_nblk.p, 0, 4, s));
        ScanArgs A{d_text, n, n_chunks, d_segs.p, nseg, std::getenv("BPE355_NOCACHE") ? 0 : 1, kv.p, pos.p,
                   cap - 1, (unsigned long long)(cap / 2), fill.p, T.recs_cache.p, rec_cap, rec_region, rec_fill.p,
                   rec_base.p, rec_n.p, pend_blocks ? S.pend.p : nullptr, pend_blocks, S.pend_nblk.p,
                   S.block_used.p, status.p};
        if (want_pos) {
            ScanCutsPos SP;
            static_cast<ScanCuts&>(SP) = SC;
            SP.rec_pos = S.rec_pos.p;
            hipLaunchKernelGGL(kern_pos, dim3(sgrid), dim3(256), kStage, s, A, D, SP);
        } else {
            hipLaunchKernelGGL(kern, dim3(sgrid), dim3(256), kStage, s, A, D, SC);
        }
        BPE_HIP(hipGetLastError());
        unsigned nblk = 0;
        to_host(&nblk, S.pend_nblk.p, 4, s);
        nblk = std::min(nblk, pend_blocks);
        pend_entries = (unsigned long long)nblk * kPendBlock;
        if (tracing) BPE_HIP(hipMemsetAsync(S.rstats.p, 0, 3 * sizeof(unsigned long long), s));
        if (nblk && !drop) {   // the pending words, resolved in place (dropout reads no word's ids)
            int r_cu = 0;
            BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&r_cu, k_enc_resolve, 256, 0));
            const unsigned long long ne = (unsigned long long)nblk * kPendBlock;
            const unsigned rgrid = (unsigned)std::min<unsigned long long>(ceil_div(ne, 256),
                                                                         (unsigned long long)std::max(1, r_cu) * std::max(1, n_cu) * 8);
            ResolveArgs RA{d_text, n, S.pend.p, S.block_used.p, ne, kv.p, pos.p, cap - 1, (unsigned long long)(cap / 2),
                           fill.p, status.p, tracing ? S.rstats.p : nullptr};
            // the LDS-cached resolve (default: 195 vs 198 ms at the bench corpus, r04h); the knob's
            // 0 runs the uncached one
            const char* rc_env = std::getenv("BPE355_ENC_RESOLVE_CACHE");
            if (!(rc_env && rc_env[0] == '0')) {
                int c_cu = 0;
                BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c_cu, k_enc_resolve_c, 256, 0));
                const unsigned cgrid = std::min<unsigned>(nblk, (unsigned)(std::max(1, c_cu) * std::max(1, n_cu)));
                hipLaunchKernelGGL(k_enc_resolve_c, dim3(cgrid), dim3(256), 0, s, RA, D, nblk);
            } else {
                hipLaunchKernelGGL(k_enc_resolve, dim3(rgrid), dim3(256), 0, s, RA, D);
            }
            BPE_HIP(hipGetLastError());
        }
        unsigned st = 0;
        to_host(&st, status.p, 4, s);
        if (st & 2u) throw Error{BPE_E_LIMIT, "a pre-token is 8 MiB or longer"};
        BPE_REQUIRE(!(st & 16u), BPE_E_HIP, "internal error: encode scan found an empty pre-token");
        if (st & 1u) {
            BPE_REQUIRE(attempt < 8, BPE_E_NOMEM, "word table overflow");
            cap *= 4;
            continue;
        }
        if (st & 256u) {   // more pre-tokens than guessed: one per byte at most
            BPE_REQUIRE(attempt < 8, BPE_E_HIP, "internal error: encode records overflow (retries)");
            BPE_REQUIRE(rec_cap < rec_cap_max, BPE_E_HIP, "internal error: encode records overflow");
            rec_cap = rec_cap_max;
            continue;
        }
        break;
    }
    if (drop) {   // every occurrence merges on its own: no word table, no resolve, no emit (dropout.hip)
        if constexpr (std::is_same<OutT, uint32_t>::value) {
            BPE_REQUIRE(want_pos, BPE_E_ARG, "encode with dropout needs the document starts");
            S.chunk_next.reserve(n_chunks);
            hipLaunchKernelGGL(k_enc_chunk_next, dim3(grid_for(n_chunks, 256)), dim3(256), 0, s, rec_n.p, rec_base.p,
                               S.rec_pos.p, n_chunks, (unsigned long long)n, S.chunk_next.p);
            BPE_HIP(hipGetLastError());
            const DropTables DT{E.pm_key, E.pm_val, E.pm_mask, E.tok2vid, E.byte2tok, E.sp_bytes, E.sp_off, E.sp_len,
                                E.sp_vid, E.n_sp};
            const DropFront F{d_text, n, n_chunks, (size_t)kChunk, T.recs_cache.p, kRecKind3, kRecSpecial, kRecPayload29,
                              S.rec_pos.p, rec_base.p, rec_n.p, S.chunk_next.p, S.cuts.p, S.chunk_cut0.p, S.cut_rec.p,
                              &cuts, docs->starts, docs->n_docs, d_out, docs->d_out};
            return dropout_emit(F, DT, *drop, S.drop, s);
        } else {
            BPE_REQUIRE(false, BPE_E_ARG, "encode with dropout writes uint32 ids");
        }
    }
    DevBuf<uint32_t>&w_slot = S.w_slot, &w_len = S.w_len;
    DevBuf<unsigned long long>& w_off = S.w_off;
    DevBuf<unsigned>& d_nw = S.d_nw;
    w_slot.reserve(cap);
    w_off.reserve(cap);
    w_len.reserve(cap);
    d_nw.reserve(1);
    BPE_HIP(hipMemsetAsync(d_nw.p, 0, 4, s));
    hipLaunchKernelGGL(k_collect, dim3(ceil_div(cap, 256 * kCollectPer)), dim3(256), 0, s, kv.p, pos.p, cap, w_slot.p,
                       w_off.p, w_len.p, d_nw.p);
    unsigned nw = 0;
    to_host(&nw, d_nw.p, 4, s);
    if (tracing) {
        unsigned long long nrec = 0, rs[3];
        to_host(&nrec, rec_fill.p, 8, s);
        to_host(rs, S.rstats.p, sizeof rs, s);
        std::fprintf(stderr, "[bpe355 encode] resolve: %llu LDS-cache hits, %llu dictionary words, %llu table words\n",
                     rs[0], rs[1], rs[2]);
        std::vector<uint32_t> used(pend_entries / kPendBlock);
        if (!used.empty()) to_host(used.data(), S.block_used.p, used.size() * 4, s);
        unsigned long long npend = 0;
        for (uint32_t u : used) npend += u;
        std::fprintf(stderr, "[bpe355 encode] %zu bytes: %llu record slots reserved, %llu pending (%zu blocks), %u table words "
                     "(%zu slots), dictionary %zu words\n", n, nrec, npend, used.size(), nw, cap, T.dict_words);
    }

    // 3. encode each word of the table once
    DevBuf<unsigned long long>&len64 = S.len64, &idoff = S.idoff;
    len64.reserve(std::max(nw, 1u));
    idoff.reserve(std::max(nw, 1u) + 1);
    DevBuf<unsigned long long>& slot_info = S.slot_info;   // every slot a record names is a word's slot
    slot_info.reserve(cap);
    BPE_HIP(hipMemsetAsync(slot_info.p, 0, cap * sizeof(unsigned long long), s));
    unsigned long long pool_n = 0;
    if (nw) {
        hipLaunchKernelGGL(k_word_len64, dim3(ceil_div(nw, 256)), dim3(256), 0, s, w_len.p, nw, len64.p);
        exclusive_sum(len64.p, idoff.p, nw, s, &S.tmp);
        unsigned long long last[2];
        to_host(&last[0], idoff.p + nw - 1, 8, s);
        to_host(&last[1], len64.p + nw - 1, 8, s);
        pool_n = last[0] + last[1];
    }
    BPE_REQUIRE(pool_n < kDictPool, BPE_E_LIMIT, "too many distinct words for one encode");
    DevBuf<uint32_t>& pool = S.pool;
    pool.reserve(std::max<unsigned long long>(pool_n, 1));
    BPE_HIP(hipMemsetAsync(status.p, 0, 4, s));
    if (nw) {
        hipLaunchKernelGGL(k_encode_words, dim3(ceil_div(nw, 256)), dim3(256), 0, s, d_text, E, w_off.p,
                           w_len.p, idoff.p, w_slot.p, nw, pool.p, slot_info.p, status.p, n);
        BPE_HIP(hipGetLastError());
    }
    // A/B knob BPE355_ENC_FINALIZE: 0 the emit reads the resolved records instead, 2 the emit's
    // count pass resolves them and stores the infos for the write pass
    const char* fin_env = std::getenv("BPE355_ENC_FINALIZE");
    const int fin_mode = fin_env ? std::atoi(fin_env) : 1;
    const bool finalize = pend_entries && fin_mode == 1;
    const bool writeback = pend_entries && fin_mode == 2;
    if (finalize) {   // pending entries: record -> ids' info
        int f_cu = 0;
        BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&f_cu, k_enc_finalize, 256, 0));
        const unsigned fgrid = (unsigned)std::min<unsigned long long>(ceil_div(pend_entries, 256),
                                                                     (unsigned long long)std::max(1, f_cu) * std::max(1, n_cu) * 8);
        hipLaunchKernelGGL(k_enc_finalize, dim3(fgrid), dim3(256), 0, s, S.pend.p, S.block_used.p, pend_entries,
                           slot_info.p, cap, D, T.dict_slots, status.p);
        BPE_HIP(hipGetLastError());
    }
    // 4. ids: the chunks' id counts, their exclusive scan, then the write pass
    DevBuf<unsigned long long>&ctot = S.ctot, &coff = S.coff;
    const size_t n_parts = n_chunks * kEmitParts;
    ctot.reserve(n_parts);
    coff.reserve(n_parts);
    EmitArgs EA{T.recs_cache.p, rec_base.p, rec_n.p, n_chunks, slot_info.p, pool.p, cap, D, T.dict_slots,
                S.pend.p, finalize ? 1 : 0, writeback ? 1 : 0, E.sp_vid, ctot.p, coff.p, status.p};
    {
        auto ck = k_enc_emit<OutT, true>;
        int c_cu = 0;
        BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c_cu, ck, 256, 0));
        const unsigned cgrid = (unsigned)std::min<size_t>(n_parts, (size_t)std::max(1, c_cu) * std::max(1, n_cu) * 2);
        hipLaunchKernelGGL(ck, dim3(cgrid), dim3(256), 0, s, EA, d_out);
        BPE_HIP(hipGetLastError());
    }
    exclusive_sum(ctot.p, coff.p, n_parts, s, &S.tmp);
    if (writeback) EA.finalized = 1;   // every pending entry holds its info now
    {
        auto wk = k_enc_emit<OutT, false>;
        int w_cu = 0;
        BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&w_cu, wk, 256, 0));
        const unsigned wgrid = (unsigned)std::min<size_t>(n_parts, (size_t)std::max(1, w_cu) * std::max(1, n_cu) * 2);
        hipLaunchKernelGGL(wk, dim3(wgrid), dim3(256), 0, s, EA, d_out);
        BPE_HIP(hipGetLastError());
    }
    if (docs) {   // the documents' id offsets: the cuts' (from the kept attempt's scan), then one gather
        if (want_cuts) {
            int o_cu = 0;
            BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o_cu, k_enc_cut_offsets, 256, 0));
            const unsigned ogrid = (unsigned)std::min<size_t>(n_parts, (size_t)std::max(1, o_cu) * std::max(1, n_cu) * 2);
            hipLaunchKernelGGL(k_enc_cut_offsets, dim3(ogrid), dim3(256), 0, s, EA, S.chunk_cut0.p, S.cut_rec.p,
                               S.cut_off.p);
            BPE_HIP(hipGetLastError());
        }
        const size_t nd = docs->n_docs + 1;
        // every start after the first a cut of its own (no empty document): document i is cut
        // i - 1 and the gather needs no table; else each document's cut, from the host
        const bool one_to_one = cuts.size() + 1 == docs->n_docs;
        if (!one_to_one) {
            std::vector<uint32_t> dc(nd);
            size_t j = 0;
            for (size_t i = 0; i < docs->n_docs; ++i) {
                const unsigned long long st = docs->starts[i];
                while (j < cuts.size() && cuts[j] < st) ++j;
                dc[i] = st == 0 ? kDocAtZero : st >= n ? kDocAtEnd : (uint32_t)j;
            }
            dc[docs->n_docs] = kDocAtEnd;
            S.doc_cut.reserve(nd);
            to_device(S.doc_cut.p, dc.data(), nd * 4, s);
        }
        hipLaunchKernelGGL(k_enc_doc_offsets, dim3(grid_for(nd, 256)), dim3(256), 0, s,
                           one_to_one ? nullptr : S.doc_cut.p, nd, S.cut_off.p,
                           coff.p, ctot.p, n_parts, docs->d_out);
        BPE_HIP(hipGetLastError());
    }
    unsigned long long last[2] = {0, 0};
    unsigned st = 0;
    to_host(&last[0], coff.p + n_parts - 1, 8, s);
    to_host(&last[1], ctot.p + n_parts - 1, 8, s);
    to_host(&st, status.p, 4, s);
    if (st & 4u) throw Error{BPE_E_KEY, "a merged token is not in the vocab"};
    BPE_REQUIRE(!(st & 96u), BPE_E_HIP, "internal error: encode records inconsistent (status " +
                                          std::to_string(st) + ")");
    if (sizeof(OutT) == 2)
        BPE_REQUIRE(!(st & 128u), BPE_E_LIMIT, "a token id does not fit np.uint16 (vocab larger than 65536)");
    const size_t total = last[0] + last[1];
    BPE_REQUIRE(total <= n, BPE_E_HIP, "encode produced more ids than input bytes");
    if (want_pos && total) {   // the spans: one more pass over the records, then (unit 1) bytes -> characters
        S.chunk_next.reserve(n_chunks);
        hipLaunchKernelGGL(k_enc_chunk_next, dim3(grid_for(n_chunks, 256)), dim3(256), 0, s, rec_n.p, rec_base.p,
                           S.rec_pos.p, n_chunks, (unsigned long long)n, S.chunk_next.p);
        BPE_HIP(hipGetLastError());
        const SpanArgs PA{S.rec_pos.p, S.chunk_next.p, S.cuts.p, S.chunk_cut0.p, E.sp_len, T.span_lens()};
        int p_cu = 0;
        BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p_cu, k_enc_emit_spans, 256, 0));
        const unsigned pgrid = (unsigned)std::min<size_t>(n_parts, (size_t)std::max(1, p_cu) * std::max(1, n_cu) * 2);
        hipLaunchKernelGGL(k_enc_emit_spans, dim3(pgrid), dim3(256), 0, s, EA, PA, (unsigned long long)n, spans->d_spans);
        BPE_HIP(hipGetLastError());
        to_host(&st, status.p, 4, s);
        BPE_REQUIRE(!(st & kSpanStatus), BPE_E_HIP, "internal error: a word's id lengths do not sum to its bytes");
        if (spans->unit == 1) {
            const size_t lead = reinterpret_cast<uintptr_t>(d_text) & 63, n_blocks = (n + lead + 63) / 64;
            S.char_cnt.reserve(n_blocks + 1);
            S.char_pre.reserve(n_blocks + 1);
            S.doc_start.reserve(docs->n_docs);
            to_device(S.doc_start.p, docs->starts, docs->n_docs * 8, s);
            BPE_HIP(hipMemsetAsync(S.char_cnt.p + n_blocks, 0, 8, s));
            hipLaunchKernelGGL(k_char_blocks, dim3(std::min<unsigned>(grid_for(n_blocks * 4, 256), 8192)), dim3(256), 0, s,
                               d_text, n, n_blocks, S.char_cnt.p);
            BPE_HIP(hipGetLastError());
            exclusive_sum(S.char_cnt.p, S.char_pre.p, n_blocks + 1, s, &S.tmp);
            hipLaunchKernelGGL(k_span_chars, dim3(grid_for(total, 256)), dim3(256), 0, s, d_text, n, S.char_pre.p,
                               n_blocks, docs->d_out, S.doc_start.p, docs->n_docs, total, spans->d_spans);
            BPE_HIP(hipGetLastError());
        }
    }
    BPE_HIP(hipStreamSynchronize(s));
    return total;
}

// ------------------------------------------------------------------ several devices
// The tokenizer for rank r on device dev: the handle itself for rank 0 on its own device, else a
// copy built from the same inputs (every rank owns its stream and record buffer, also when
// ranks share a device in tests).  The caller has made `dev` current.
bpe_tokenizer& tok_for_rank(bpe_tokenizer& T, int r, int dev) {
    if (r == 0 && dev == T.device) return T;
    const long long key = ((long long)r << 8) | dev;
    std::lock_guard<std::mutex> g(T.copies_m);
    for (auto& c : T.copies)
        if (c.first == key) return *c.second;
    auto U = std::make_unique<bpe_tokenizer>();
    build_tokenizer(*U, reinterpret_cast<const uint8_t*>(T.vblob.data()), T.vblob.size(),
                    reinterpret_cast<const uint8_t*>(T.mblob.data()), T.mblob.size(), T.sp_in);
    U->device = dev;
    T.copies.emplace_back(key, std::move(U));
    return *T.copies.back().second;
}

// g + 1 cut points of text[0, n) for separate encodes whose ids concatenate to encode(text): safe
// split points (a U+0020 between ASCII non-space bytes: the pre-tokens on both sides are those
// of the whole, pretok.h) that no occurrence of any special token spans, so re.split's leftmost
// matches (tokenizer.py:63-66) are those of the whole text too.  A slab with no such point is
// empty (its neighbour takes the text).
std::vector<size_t> encode_cuts(const uint8_t* t, size_t n, int g, const std::vector<std::string>& sp) {
    std::vector<size_t> cut{0};
    for (int r = 1; r < g; ++r) {
        size_t p = n / (size_t)g * (size_t)r;
        for (;;) {
            p = p >= 1 ? bpe_safe_split(t, n, p) : 0;
            if (p == 0 || p <= cut.back()) { p = cut.back(); break; }
            bool spans = false;
            for (const auto& x : sp) {
                const size_t L = x.size();
                for (size_t q = p + 1 > L ? p + 1 - L : 0; q < p && q + L <= n && !spans; ++q)
                    spans = std::memcmp(t + q, x.data(), L) == 0;
                if (spans) break;
            }
            if (!spans) break;
            --p;   // a special spans it: look further back
        }
        cut.push_back(p);
    }
    cut.push_back(n);
    return cut;
}

size_t encode_gpus(bpe_tokenizer& T, const uint8_t* utf8, size_t n, uint32_t* ids_out, int n_gpus) {
    int cur = 0;
    BPE_HIP(hipGetDevice(&cur));
    const std::vector<int> dev = pick_devices(n_gpus);
    const int g = (int)dev.size();
    const std::vector<size_t> cut = encode_cuts(utf8, n, g, T.specials);
    std::vector<std::vector<uint32_t>> ids(g);
    std::vector<std::exception_ptr> errs(g);
    auto work = [&](int r) {
        try {
            BPE_HIP(hipSetDevice(dev[r]));
            const size_t len = cut[r + 1] - cut[r];
            if (len == 0) return;
            bpe_tokenizer& U = tok_for_rank(T, r, dev[r]);
            DevBuf<uint8_t> d_text(len);
            DevBuf<uint32_t> d_out(len);
            BPE_HIP(hipMemcpyAsync(d_text.p, utf8 + cut[r], len, hipMemcpyHostToDevice, U.stream));
            const size_t m = encode_device(U, d_text.p, len, d_out.p, U.stream);
            ids[r].resize(m);
            if (m) BPE_HIP(hipMemcpyAsync(ids[r].data(), d_out.p, m * 4, hipMemcpyDeviceToHost, U.stream));
            BPE_HIP(hipStreamSynchronize(U.stream));
        } catch (...) {
            errs[r] = std::current_exception();
        }
    };
    std::vector<std::thread> th;
    for (int r = 1; r < g; ++r) th.emplace_back(work, r);
    work(0);
    for (auto& x : th) x.join();
    (void)hipSetDevice(cur);
    for (auto& e : errs)   // the earliest slab's error: the one encode(text) would raise first
        if (e) std::rethrow_exception(e);
    size_t m = 0;
    for (int r = 0; r < g; ++r) {
        if (!ids[r].empty()) std::memcpy(ids_out + m, ids[r].data(), ids[r].size() * 4);
        m += ids[r].size();
    }
    return m;
}

// encode_batch's document starts, checked, as encode_device's cuts
std::vector<unsigned long long> batch_cuts(const uint64_t* starts, size_t n_docs, size_t n) {
    BPE_REQUIRE(n_docs == 0 || starts, BPE_E_ARG, "NULL doc_starts");
    BPE_REQUIRE(n_docs > 0 || n == 0, BPE_E_ARG, "text without a document");
    BPE_REQUIRE(n_docs < (1ull << 60), BPE_E_ARG, "too many documents");
    BPE_REQUIRE(n_docs == 0 || starts[0] == 0, BPE_E_ARG, "doc_starts[0] must be 0");
    for (size_t i = 1; i < n_docs; ++i)
        BPE_REQUIRE(starts[i] >= starts[i - 1], BPE_E_ARG, "doc_starts must not decrease");
    BPE_REQUIRE(n_docs == 0 || starts[n_docs - 1] <= n, BPE_E_ARG, "a document starts past the end of the text");
    return std::vector<unsigned long long>(starts, starts + n_docs);
}

}  // namespace

hipStream_t tokenizer_stream(bpe_tokenizer* tok) { return tok->stream; }

size_t encode_dropout_device(bpe_tokenizer* tok, const uint8_t* d_text, size_t n, const uint64_t* doc_starts,
                             size_t n_docs, const DropParams& P, uint32_t* d_ids, unsigned long long* d_id_offsets,
                             hipStream_t s) {
    const std::vector<unsigned long long> cuts = batch_cuts(doc_starts, n_docs, n);
    for (size_t i = 0; i < n_docs; ++i)
        BPE_REQUIRE(((i + 1 < n_docs ? doc_starts[i + 1] : (uint64_t)n) - doc_starts[i]) >> 32 == 0, BPE_E_LIMIT,
                    "a document of 2^32 bytes or more");
    if (!s) s = tok->stream;
    if (n == 0) {   // empty documents only: every offset is 0
        BPE_HIP(hipMemsetAsync(d_id_offsets, 0, (n_docs + 1) * sizeof(uint64_t), s));
        BPE_HIP(hipStreamSynchronize(s));
        return 0;
    }
    const DocStarts docs{doc_starts, n_docs, d_id_offsets};
    return encode_device(*tok, d_text, n, d_ids, s, cuts, &docs, nullptr, &P);
}

namespace {

template <class F>
int guarded_enc(F&& f) {
    try {
        f();
        set_error(0, "");
        return BPE_OK;
    } catch (const Error& e) {
        set_error(e.code, e.msg);
        return e.code;
    } catch (const std::bad_alloc&) {
        set_error(BPE_E_NOMEM, "host allocation failed");
        return BPE_E_NOMEM;
    }
}

// ------------------------------------------------------------------ file -> uint16 ids, overlapped
// encode.py:31-37 for a regular file.  A reader thread streams the file into HBM in kReadSlab
// slabs; as they land, the main thread validates the loaded prefix (strict UTF-8, exactly as one
// pass over the whole text), counts its characters to place the piece starts (every
// chars_per_piece-th character, f.read(K)), encodes the pieces that are complete and validated
// straight to uint16 in the tokenizer's kept buffer, and hands their ids to a copier thread that
// moves them into ids_out while the next region is read and encoded.  A text with a carriage
// return (universal newlines move every later piece start) is redone in one serial pass once
// it has been read.  phase_ms: busy time of the reader, of validation + counting, of the encodes
// and of the copier (they overlap).
constexpr size_t kReadSlab = 1ull << 30;        // a multiple of the counting block (64 KiB)
constexpr size_t kMaxRegion = 3ull << 30;       // bytes one encode takes at most
constexpr size_t kLastRegion = 256ull << 20;    // bytes of the last region (the copy tail)
constexpr size_t kMinRegion = 64ull << 20;      // bytes a region takes at least while the file arrives

size_t env_size(const char* name, size_t dflt) {   // test knobs: small slabs and regions
    const char* e = std::getenv(name);
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? (size_t)v : dflt;
}

size_t encode_file_pipelined(bpe_tokenizer& T, const Source& src, size_t K, uint16_t* ids_out, size_t cap, int dev,
                             double* ph) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    auto& S = T.sc;
    const hipStream_t s = T.stream;
    const size_t n = src.size;
    if (n == 0) return 0;
    const auto t_call = clk::now();
    const size_t read_slab = std::max<size_t>(1, env_size("BPE355_READ_SLAB", kReadSlab) >> 16) << 16;
    const size_t max_region = env_size("BPE355_ENC_REGION", kMaxRegion);
    const size_t last_region = std::min(max_region, env_size("BPE355_ENC_LAST_REGION", kLastRegion));
    const size_t min_region = std::min(max_region, env_size("BPE355_ENC_MIN_REGION", kMinRegion));
    // per-region lines (range, ids, pieces, ms; then the call's clock in ms at: the slab seen, its
    // validation + counting done, the encode done) appended to the file BPE355_ENC_TRACE names,
    // and one line per slab read and per copy (start, end)
    const char* trace_path = std::getenv("BPE355_ENC_TRACE");
    FILE* const trace = trace_path ? std::fopen(trace_path, "a") : nullptr;
    struct Closer { FILE* f; ~Closer() { if (f) std::fclose(f); } } trace_closer{trace};
    S.text.reserve(n);
    S.ids16.reserve(n);   // ids <= bytes
    uint8_t* const text = S.text.p;

    // reader
    std::mutex m;
    std::condition_variable cv;
    size_t loaded = 0;
    bool read_done = false;
    std::atomic<bool> stop{false};   // an error downstream: read no further
    std::exception_ptr read_err;
    // reader and copier threads, each (measured at 11.9 GB, r04: 8 threads 492-508 ms per call,
    // 4 threads 1.96-2.0 s before the region encode got fast; r03, with a 430 ms encode phase: 4
    // threads 593-648 ms, 8: 713-749, 16: 810-858)
    const int io_n = (int)env_size("BPE355_ENC_IO_THREADS", 8);
    // host threads of each region's copy-out (BPE355_ENC_COPY_THREADS): 4 leave the host cores the
    // encoder's own thread needs while 8 readers run (r04zc, 11.9 GB: 4 threads 358-365 ms per warm
    // call, 8 376-451, 2 442-446)
    const int copy_n = (int)env_size("BPE355_ENC_COPY_THREADS", 4);
    // experiment knob: BPE355_ENC_OVERLAP=0 reads the whole file before the first encode
    const char* ov = std::getenv("BPE355_ENC_OVERLAP");
    const bool overlap_read = !(ov && ov[0] == '0');
    // test knob: the read fails once it reaches this byte offset (an EIO or a file truncated
    // while it is read)
    const size_t fail_at = env_size("BPE355_TEST_READ_FAIL_AT", 0);
    std::thread reader([&] {
        const auto t0 = clk::now();
        try {
            for (size_t off = 0; off < n && !stop.load(); off += read_slab) {
                const size_t len = std::min(read_slab, n - off);
                if (fail_at && off + len >= fail_at)
                    throw Error{BPE_E_IO, "read failed (injected by BPE355_TEST_READ_FAIL_AT)"};
                const double r0 = since(t_call);
                stage_to_device(src, off, len, text + off, dev, io_n);
                if (trace) {
                    std::lock_guard<std::mutex> g(m);
                    std::fprintf(trace, "read %zu %zu at %.1f %.1f\n", off, off + len, r0, since(t_call));
                }
                std::lock_guard<std::mutex> g(m);
                loaded = off + len;
                cv.notify_all();
            }
        } catch (...) {
            std::lock_guard<std::mutex> g(m);
            read_err = std::current_exception();
        }
        std::lock_guard<std::mutex> g(m);
        read_done = true;
        ph[0] = since(t0);
        cv.notify_all();
    });
    // copier: a queue of regions copied out in order by one thread (each copy fans out over io_n
    // threads), so the encoder never waits for one region's copy before it starts the next
    // (r04za timeline: waiting for the previous copy held the encoder 13-40 ms per region)
    std::mutex qm;
    std::condition_variable qcv;
    std::deque<std::pair<size_t, size_t>> cq;
    bool cq_closed = false;
    std::exception_ptr copy_err;
    std::thread copier([&] {
        for (;;) {
            std::pair<size_t, size_t> job;
            {
                std::unique_lock<std::mutex> g(qm);
                qcv.wait(g, [&] { return !cq.empty() || cq_closed; });
                if (cq.empty()) return;
                job = cq.front();
                cq.pop_front();
            }
            if (copy_err || stop.load()) continue;   // after an error: drain without copying
            const auto t0 = clk::now();
            try {
                device_to_host(reinterpret_cast<const uint8_t*>(S.ids16.p + job.first), 2 * job.second,
                               reinterpret_cast<uint8_t*>(ids_out + job.first), dev, copy_n);
            } catch (...) {
                copy_err = std::current_exception();
            }
            ph[3] += since(t0);
            if (trace) {
                std::lock_guard<std::mutex> g(m);
                std::fprintf(trace, "copy %zu ids at %.1f %.1f\n", job.second,
                             std::chrono::duration<double, std::milli>(t0 - t_call).count(), since(t_call));
            }
        }
    });
    auto copy_close = [&] {
        {
            std::lock_guard<std::mutex> g(qm);
            cq_closed = true;
        }
        qcv.notify_all();
        if (copier.joinable()) copier.join();
    };
    auto copy_wait = [&] {   // every queued copy done (then no more can be queued)
        copy_close();
        if (copy_err) std::rethrow_exception(copy_err);
    };
    auto copy_start = [&](size_t at, size_t cnt) {
        {
            std::lock_guard<std::mutex> g(qm);
            cq.emplace_back(at, cnt);
        }
        qcv.notify_one();
    };
    auto finish_threads = [&] {
        stop.store(true);
        {
            std::unique_lock<std::mutex> g(m);
            cv.wait(g, [&] { return read_done; });
        }
        if (reader.joinable()) reader.join();
        copy_close();
    };

    size_t k_done = 0;
    bool serial = false;   // a carriage return: redo in one pass
    try {
        ValidatePass V;
        V.begin(text, n, s);
        std::vector<uint64_t> starts;      // piece starts found so far (global offsets)
        size_t counted = 0, enc_done = 0, next_piece = 1;   // starts[0] == 0
        uint64_t chars = 0;
        size_t seen = 0;
        while (enc_done < n) {
            size_t L;
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return (overlap_read && loaded > seen) || read_done; });
                if (read_err) std::rethrow_exception(read_err);
                L = loaded;
            }
            seen = L;
            const auto t1 = clk::now();
            const double t_seen = since(t_call);
            const size_t vend = V.prefix(L);
            const size_t cend = L == n ? n : L / 65536 * 65536;
            if (cend > counted) {
                chars += piece_starts_range(text + counted, cend - counted, K, chars, counted, s, starts, &S.piece);
                counted = cend;
            }
            unsigned long long err = 0;
            bool cr = false;
            V.finish(&err, &cr);
            ph[1] += since(t1);
            const double t_valid = since(t_call);
            if (err != ~0ULL)
                throw Error{BPE_E_UTF8, "'utf-8' codec can't decode byte at position " + std::to_string(err)};
            if (cr) { serial = true; break; }
            // encode the complete pieces inside the validated and counted prefix, at most
            // kMaxRegion at a time, each region ending at a piece start (or the end)
            const size_t ready = std::min(vend, counted);
            auto region_end = [&](size_t from) -> size_t {
                // once the whole text is in, the last region is kept short (at most last_region
                // bytes): its ids' copy is the one step nothing overlaps
                size_t span = max_region;
                if (ready == n) {
                    if (n - from <= last_region) return n;
                    span = std::min(max_region, n - from - last_region);
                }
                size_t lim = from;
                for (size_t i = next_piece; i < starts.size() && starts[i] <= std::min(ready, from + span); ++i)
                    lim = starts[i];
                if (lim == from && ready == n)   // a piece longer than kMaxRegion: whole
                    lim = next_piece < starts.size() ? starts[next_piece] : n;
                // while the file is still arriving, a short leftover (the piece cut by a slab end)
                // waits for the next slab instead of costing an encode call of its own
                if (ready < n && lim - from < min_region) return from;
                return lim;
            };
            for (size_t e_end = region_end(enc_done); e_end > enc_done; e_end = region_end(enc_done)) {
                std::vector<unsigned long long> cuts;
                for (; next_piece < starts.size() && starts[next_piece] < e_end; ++next_piece)
                    cuts.push_back(starts[next_piece] - enc_done);
                if (next_piece < starts.size() && starts[next_piece] == e_end) ++next_piece;
                const auto t2 = clk::now();
                const size_t kk = encode_device(T, text + enc_done, e_end - enc_done, S.ids16.p + k_done, s, cuts);
                const double ems = since(t2);
                ph[2] += ems;
                if (trace) {
                    std::lock_guard<std::mutex> g(m);
                    std::fprintf(trace, "region %zu %zu ids %zu pieces %zu ms %.1f loaded %zu at %.1f %.1f %.1f\n", enc_done,
                                 e_end, kk, cuts.size() + 1, ems, seen, t_seen, t_valid, since(t_call));
                    std::fflush(trace);
                }
                BPE_REQUIRE(k_done + kk <= cap, BPE_E_ARG, "ids_out holds " + std::to_string(cap) +
                                                              " ids, the file encodes to more");
                copy_start(k_done, kk);
                k_done += kk;
                enc_done = e_end;
            }
        }
        copy_wait();
    } catch (...) {
        finish_threads();
        throw;
    }
    if (serial) {   // the rest of the file first; on a read error both threads are joined first
        std::exception_ptr e;
        {
            std::unique_lock<std::mutex> g(m);
            cv.wait(g, [&] { return read_done; });
            e = read_err;
        }
        if (e) {
            finish_threads();
            std::rethrow_exception(e);
        }
    }
    finish_threads();
    if (copy_err) std::rethrow_exception(copy_err);
    if (!serial) return k_done;

    // universal newlines: one pass over the whole text, as read
    const auto t1 = clk::now();
    size_t mlen = 0;
    const uint8_t* t2 = prepare_text(text, n, S.text2, &mlen, s);
    const std::vector<uint64_t> starts = utf8_piece_starts(t2, mlen, K, s);
    ph[1] += since(t1);
    const auto te = clk::now();
    const std::vector<unsigned long long> cuts(starts.begin(), starts.end());
    const size_t kk = mlen ? encode_device(T, t2, mlen, S.ids16.p, s, cuts) : 0;
    ph[2] += since(te);
    BPE_REQUIRE(kk <= cap, BPE_E_ARG, "ids_out holds " + std::to_string(cap) + " ids, the file encodes to " +
                                         std::to_string(kk));
    const auto tc = clk::now();
    if (kk) device_to_host(reinterpret_cast<const uint8_t*>(S.ids16.p), 2 * kk, reinterpret_cast<uint8_t*>(ids_out),
                           dev, io_threads());
    ph[3] += since(tc);
    return kk;
}

// ------------------------------------------------------------------ many files -> one token file
// The dataset encoder (bpe_tok_encode_files): encode_file's result for every file, concatenated,
// without holding anything proportional to a file in HBM or in host memory.
//
// Read grid.  A reader thread reads each file's raw bytes in consecutive ranges of exactly W =
// window_bytes (the last one shorter) into a ring of two raw buffers, one range ahead of the
// main thread.  Carry.  Of a range's end, bpe_window_holdback bytes (an incomplete UTF-8
// character, a final \r that may be half of \r\n) wait and are put in front of the next range,
// so every range that is decoded ends on a character and never inside \r\n: prepare_text on it
// gives exactly the bytes the text-mode read of the whole file gives for it, and its error
// position plus the range's file offset is the position in the file.  The translated bytes are
// appended to the text buffer behind the carried text; piece_starts_range, with the file's
// running character count, finds the piece starts among the new bytes.  Everything before the
// last piece start is a run of whole pieces and is encoded with the starts as cuts; the bytes from
// that start on are the next buffer's carry, moved to the front device to device (at the end of
// the file everything is encoded).  A window edge is thus never a piece edge, and a special token
// that spans one is matched like any other.  With no piece start in the buffer the whole buffer
// is carried and the buffer grows by one window: a piece longer than a window.
//
// Device memory of the call (bpe_dataset_stats.device_bytes reports the sum): 2 raw buffers of
// W + 32; the text buffer of carry + W + 64, carry < the bytes of one piece; its carry moves
// through a second buffer of at most the carry only when source and destination overlap; 2 id
// buffers of sizeof(OutT) x the text buffer's size; 8 MiB of separator positions; the id table;
// while a window with a \r is translated, prepare_text's three arrays of its size.
//
// A writer thread copies each region's ids to the host and pwrites them at their stream offset
// while the next region is decoded and encoded (the id ring has two buffers for that).  The
// histogram and the separator search run on the region's ids right after its emit.
constexpr size_t kDatasetWindow = 1ull << 30;
constexpr size_t kRawSlack = 16;            // in front of a raw buffer: the held-back bytes go there
constexpr size_t kDatasetPosCap = 1u << 20; // separator positions one search returns at most

void pwrite_all(int fd, const void* p, size_t n, uint64_t off, const std::string& what) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    size_t done = 0;
    while (done < n) {
        const ssize_t r = ::pwrite(fd, b + done, n - done, (off_t)(off + done));
        if (r < 0) {
            if (errno == EINTR) continue;
            throw Error{BPE_E_IO, "cannot write " + what, errno};
        }
        done += (size_t)r;
    }
}

template <class OutT>
void encode_files_pipelined(bpe_tokenizer& T, const char* const* paths, size_t n_paths, int out_fd, int idx_fd,
                            const bpe_dataset_opts& O, uint64_t* file_off, uint64_t* counts, size_t n_counts,
                            bpe_dataset_stats& st, int dev) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    auto& S = T.sc;
    auto& D = T.sc.ds;
    const hipStream_t s = T.stream;
    const size_t K = O.chars_per_piece;
    const size_t W = O.window_bytes ? O.window_bytes : kDatasetWindow;
    const int io_n = (int)env_size("BPE355_ENC_IO_THREADS", 8);
    const int copy_n = (int)env_size("BPE355_ENC_COPY_THREADS", 4);
    // test knob: a small position buffer, so that a dense region is searched in several parts
    const size_t pos_cap = std::max<size_t>(16, env_size("BPE355_DS_POS_CAP", kDatasetPosCap));
    for (auto& r : D.raw) r.reserve(W + 2 * kRawSlack);
    D.text.reserve(W + 64);
    if (O.has_separator) D.pos.reserve(pos_cap);
    if (counts) {
        D.counts.reserve(n_counts);
        BPE_HIP(hipMemsetAsync(D.counts.p, 0, n_counts * 8, s));
    }

    // ---- reader: one range ahead
    struct Win {
        size_t file = 0, off = 0, len = 0;
        bool eof = false;
        uint8_t tail[4] = {0, 0, 0, 0};
        unsigned tail_n = 0;
        int slot = -1;
    };
    std::mutex m;
    std::condition_variable cv;
    std::deque<Win> ready;
    bool raw_free[2] = {true, true};
    bool read_done = false;
    std::atomic<bool> stop{false};
    std::exception_ptr read_err;
    double read_ms = 0;
    std::thread reader([&] {
        double busy = 0;
        try {
            size_t seq = 0;
            for (size_t f = 0; f < n_paths && !stop.load(); ++f) {
                const Source src = Source::open_path(paths[f]);
                if (src.size == 0) {   // no ids; the main thread closes the file's id range
                    Win w;
                    w.file = f;
                    w.eof = true;
                    std::lock_guard<std::mutex> g(m);
                    ready.push_back(w);
                    cv.notify_all();
                    continue;
                }
                for (size_t off = 0; off < src.size && !stop.load(); off += W) {
                    Win w;
                    w.file = f;
                    w.off = off;
                    w.len = std::min(W, src.size - off);
                    w.eof = off + w.len == src.size;
                    w.slot = (int)(seq++ & 1);
                    {
                        std::unique_lock<std::mutex> g(m);
                        cv.wait(g, [&] { return raw_free[w.slot] || stop.load(); });
                        if (stop.load()) break;
                        raw_free[w.slot] = false;
                    }
                    const auto t0 = clk::now();
                    stage_to_device(src, off, w.len, D.raw[w.slot].p + kRawSlack, dev, io_n);
                    w.tail_n = (unsigned)std::min<size_t>(4, w.len);
                    src.read(off + w.len - w.tail_n, w.tail_n, w.tail);
                    busy += since(t0);
                    std::lock_guard<std::mutex> g(m);
                    ready.push_back(w);
                    cv.notify_all();
                }
            }
        } catch (...) {
            std::lock_guard<std::mutex> g(m);
            read_err = std::current_exception();
        }
        std::lock_guard<std::mutex> g(m);
        read_ms = busy;
        read_done = true;
        cv.notify_all();
    });

    // ---- writer: ids of a region -> host -> the output file at their stream offset
    struct Job { int slot; size_t count; uint64_t at; };
    std::mutex qm;
    std::condition_variable qcv;
    std::deque<Job> jobs;
    bool ids_free[2] = {true, true};
    bool jobs_closed = false;
    std::exception_ptr write_err;
    double write_ms = 0;
    std::thread writer([&] {
        std::vector<uint8_t> host;
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> g(qm);
                qcv.wait(g, [&] { return !jobs.empty() || jobs_closed; });
                if (jobs.empty()) return;
                j = jobs.front();
                jobs.pop_front();
            }
            const auto t0 = clk::now();
            bool failed;
            {
                std::lock_guard<std::mutex> g(qm);
                failed = (bool)write_err;
            }
            if (!failed && !stop.load()) {
                try {
                    const size_t bytes = j.count * sizeof(OutT);
                    if (host.size() < bytes) host.resize(bytes);
                    device_to_host(D.ids[j.slot].p, bytes, host.data(), dev, copy_n);
                    pwrite_all(out_fd, host.data(), bytes, j.at * sizeof(OutT), "the token file");
                } catch (...) {
                    std::lock_guard<std::mutex> g(qm);
                    write_err = std::current_exception();
                }
            }
            std::lock_guard<std::mutex> g(qm);
            write_ms += since(t0);
            ids_free[j.slot] = true;
            qcv.notify_all();
        }
    });
    auto join_all = [&] {
        stop.store(true);
        {
            std::lock_guard<std::mutex> g(m);
            cv.notify_all();
        }
        if (reader.joinable()) reader.join();
        {
            std::lock_guard<std::mutex> g(qm);
            jobs_closed = true;
        }
        qcv.notify_all();
        if (writer.joinable()) writer.join();
    };

    uint64_t k_done = 0, n_sep = 0;
    try {
        size_t carry = 0;          // translated bytes at the front of the text buffer
        uint64_t chars = 0;        // characters of the current file before the bytes not yet counted
        unsigned hold_prev = 0;    // raw bytes held back from the previous range
        uint8_t held[4] = {0, 0, 0, 0};
        int id_slot = 0;
        std::vector<uint64_t> starts;
        std::vector<unsigned long long> hpos;
        if (file_off) file_off[0] = 0;
        for (;;) {
            Win w;
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return !ready.empty() || read_done; });
                if (ready.empty()) {
                    if (read_err) std::rethrow_exception(read_err);
                    break;
                }
                w = ready.front();
                ready.pop_front();
            }
            size_t total = carry;
            if (w.len) {
                ++st.n_windows;
                st.n_bytes += w.len;
                st.max_window_bytes = std::max<uint64_t>(st.max_window_bytes, w.len);
                const auto t1 = clk::now();
                const unsigned hold = (unsigned)bpe_window_holdback(w.tail, w.tail_n, w.eof ? 1 : 0);
                uint8_t* const in = D.raw[w.slot].p + kRawSlack - hold_prev;
                if (hold_prev) to_device(in, held, hold_prev, s);
                const size_t nin = hold_prev + w.len - hold;
                size_t mlen = 0;
                DevBuf<uint8_t> nl;   // the translated copy of a window that holds a \r
                DevBuf<uint8_t> fixed;   // the repaired copy of a range that fails validation (non-strict)
                const uint8_t* t = nullptr;
                try {
                    t = prepare_text(in, nin, nl, &mlen, s);
                } catch (const Error& e) {
                    const size_t p = e.msg.find("position ");
                    if (e.code != BPE_E_UTF8 || p == std::string::npos) throw;
                    if (!T.errors)
                        throw Error{BPE_E_UTF8, "'utf-8' codec can't decode byte at position " +
                                                    std::to_string(std::stoull(e.msg.substr(p + 9)) + (w.off - hold_prev)) +
                                                    " of " + paths[w.file]};
                    // The range ends where bpe_window_holdback cut it: what is held back is a proper
                    // prefix of a well-formed sequence, a unit that could still grow, and every unit
                    // before it is decided whatever follows.  So the ranges' repairs are the file's.
                    bpe_utf8_stats ws{0, 0, ~0ULL};
                    size_t fn = 0;
                    t = repair_text(in, nin, T.errors, fixed, &fn, &ws, s);
                    if (T.fix_total.first == ~0ULL && ws.first != ~0ULL) T.fix_first_file = w.file;
                    utf8_stats_add(T.fix_total, ws, w.off - hold_prev);
                    T.fix_file_units[w.file] += ws.n_units;
                    mlen = fn;
                    if (fn) t = prepare_text(t, fn, nl, &mlen, s);
                }
                if (D.text.n < carry + mlen + 64) {   // a piece longer than the buffer: grow, keep the carry
                    DevBuf<uint8_t> nb(carry + mlen + 64);
                    if (carry) BPE_HIP(hipMemcpyAsync(nb.p, D.text.p, carry, hipMemcpyDeviceToDevice, s));
                    BPE_HIP(hipStreamSynchronize(s));
                    D.text = std::move(nb);
                    ++st.n_grows;
                }
                BPE_HIP(hipMemcpyAsync(D.text.p + carry, t, mlen, hipMemcpyDeviceToDevice, s));
                starts.clear();
                chars += piece_starts_range(D.text.p + carry, mlen, K, chars, carry, s, starts, &S.piece);
                BPE_HIP(hipStreamSynchronize(s));   // the raw buffer has been copied out of
                nl.release();
                {
                    std::lock_guard<std::mutex> g(m);
                    raw_free[w.slot] = true;
                    cv.notify_all();
                }
                hold_prev = hold;
                for (unsigned i = 0; i < hold; ++i) held[i] = w.tail[w.tail_n - hold + i];
                total = carry + mlen;
                st.decode_ms += since(t1);
            }
            // whole pieces: up to the last piece start in the buffer, or to the end of the file
            const size_t e_end = w.eof ? total : (starts.empty() || !w.len ? 0 : (size_t)starts.back());
            if (e_end) {
                std::vector<unsigned long long> cuts;
                for (const uint64_t c : starts)
                    if (c > 0 && c < e_end) cuts.push_back(c);
                {
                    std::unique_lock<std::mutex> g(qm);
                    qcv.wait(g, [&] { return ids_free[id_slot] || (bool)write_err; });
                    if (write_err) std::rethrow_exception(write_err);
                    ids_free[id_slot] = false;
                }
                struct SlotGuard {   // an encode that throws gives the slot back
                    std::mutex& qm; bool& flag; bool armed = true;
                    ~SlotGuard() { if (armed) { std::lock_guard<std::mutex> g(qm); flag = true; } }
                } guard{qm, ids_free[id_slot]};
                D.ids[id_slot].reserve(e_end * sizeof(OutT) + 64);
                OutT* const ids = reinterpret_cast<OutT*>(D.ids[id_slot].p);
                const auto t2 = clk::now();
                const size_t kk = encode_device(T, D.text.p, e_end, ids, s, cuts);
                st.encode_ms += since(t2);
                st.n_pieces += cuts.size() + 1;
                const auto t3 = clk::now();
                if (counts) ids_histogram(ids, kk, (int)sizeof(OutT), D.counts.p, n_counts, s, D.stat);
                if (O.has_separator) {
                    // a part of at most pos_cap ids has at most pos_cap matches: the whole region
                    // in one search when its matches fit, else part by part
                    size_t found = ids_find(ids, kk, (int)sizeof(OutT), O.separator_id, k_done, D.pos.p, pos_cap, s, D.stat);
                    auto flush_pos = [&](size_t cnt) {
                        if (!cnt) return;
                        hpos.resize(cnt);
                        to_host(hpos.data(), D.pos.p, cnt * 8, s);
                        pwrite_all(idx_fd, hpos.data(), cnt * 8, n_sep * 8, "the index file");
                        n_sep += cnt;
                    };
                    if (found <= pos_cap) {
                        flush_pos(found);
                    } else {
                        for (size_t lo = 0; lo < kk; lo += pos_cap) {
                            found = ids_find(ids + lo, std::min(pos_cap, kk - lo), (int)sizeof(OutT), O.separator_id,
                                             k_done + lo, D.pos.p, pos_cap, s, D.stat);
                            flush_pos(found);
                        }
                    }
                }
                st.stats_ms += since(t3);
                {
                    std::lock_guard<std::mutex> g(qm);
                    guard.armed = false;
                    jobs.push_back(Job{id_slot, kk, k_done});
                }
                qcv.notify_all();
                k_done += kk;
                id_slot ^= 1;
                // the carry to the front
                const size_t rest = total - e_end;
                if (rest) {
                    if (rest <= e_end) {
                        BPE_HIP(hipMemcpyAsync(D.text.p, D.text.p + e_end, rest, hipMemcpyDeviceToDevice, s));
                    } else {
                        D.move.reserve(rest);
                        BPE_HIP(hipMemcpyAsync(D.move.p, D.text.p + e_end, rest, hipMemcpyDeviceToDevice, s));
                        BPE_HIP(hipMemcpyAsync(D.text.p, D.move.p, rest, hipMemcpyDeviceToDevice, s));
                    }
                    BPE_HIP(hipStreamSynchronize(s));
                }
                carry = rest;
            } else {
                carry = total;
            }
            if (w.eof) {
                carry = 0;
                chars = 0;
                hold_prev = 0;
                if (file_off) file_off[w.file + 1] = k_done;
            }
        }
        if (counts) to_host(counts, D.counts.p, n_counts * 8, s);
    } catch (...) {
        join_all();
        throw;
    }
    {   // every queued write done
        std::lock_guard<std::mutex> g(qm);
        jobs_closed = true;
    }
    qcv.notify_all();
    writer.join();
    reader.join();
    if (write_err) std::rethrow_exception(write_err);
    st.n_ids = k_done;
    st.n_separators = n_sep;
    st.read_ms = read_ms;
    st.write_ms = write_ms;
    st.device_bytes = D.raw[0].bytes() + D.raw[1].bytes() + D.text.bytes() + D.move.bytes() + D.ids[0].bytes() +
                      D.ids[1].bytes() + D.pos.bytes() + (counts ? D.counts.bytes() : 0);
}

}  // namespace
}  // namespace bpe

extern "C" {

int bpe_tok_create(const uint8_t* vocab_blob, size_t vocab_n, const uint8_t* merges_blob, size_t merges_n,
                   const char* const* specials, int n_specials, bpe_tokenizer** out) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(out && vocab_blob && merges_blob, BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(n_specials >= 0 && (n_specials == 0 || specials), BPE_E_ARG, "bad specials");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw bpe::Error{BPE_E_HIP, "no HIP device visible (libbpe355 needs an MI355X / gfx950 GPU)"};
        std::vector<std::string> sp;
        for (int i = 0; i < n_specials; ++i) {
            BPE_REQUIRE(specials[i], BPE_E_ARG, "null special");
            sp.emplace_back(specials[i]);
        }
        auto T = std::make_unique<bpe_tokenizer>();
        bpe::build_tokenizer(*T, vocab_blob, vocab_n, merges_blob, merges_n, sp);
        T->vblob.assign(reinterpret_cast<const char*>(vocab_blob), vocab_n);
        T->mblob.assign(reinterpret_cast<const char*>(merges_blob), merges_n);
        T->sp_in = sp;
        BPE_HIP(hipGetDevice(&T->device));
        *out = T.release();
    });
}

int64_t bpe_tok_special_id(const bpe_tokenizer* tok, int i) {
    if (!tok || i < 0 || i >= (int)tok->special_vid.size()) return -1;
    return tok->special_vid[i];
}

int bpe_tok_encode(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, uint32_t* ids_out, size_t cap,
                   size_t* n_out) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && (n == 0 || (utf8 && ids_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(cap >= n, BPE_E_ARG, "ids_out capacity must be >= input bytes");
        *n_out = 0;
        if (n == 0) return;
        bpe::DevBuf<uint8_t> d_text(n);
        bpe::DevBuf<uint32_t> d_out(n);
        BPE_HIP(hipMemcpyAsync(d_text.p, utf8, n, hipMemcpyHostToDevice, tok->stream));
        const size_t m = bpe::encode_device(*tok, d_text.p, n, d_out.p, tok->stream);
        if (m) BPE_HIP(hipMemcpyAsync(ids_out, d_out.p, m * 4, hipMemcpyDeviceToHost, tok->stream));
        BPE_HIP(hipStreamSynchronize(tok->stream));
        *n_out = m;
    });
}

int bpe_tok_encode_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, uint32_t* d_out,
                          size_t* n_out, void* hip_stream) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && (n == 0 || (d_utf8 && d_out)), BPE_E_ARG, "NULL argument");
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : tok->stream;
        *n_out = bpe::encode_device(*tok, d_utf8, n, d_out, s);
    });
}

int bpe_tok_encode_chunks_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* starts,
                                 size_t n_starts, uint32_t* d_out, size_t* n_out, void* hip_stream) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && (n == 0 || (d_utf8 && d_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(n_starts == 0 || starts, BPE_E_ARG, "NULL starts");
        std::vector<unsigned long long> cuts(starts, starts + n_starts);
        for (size_t i = 1; i < cuts.size(); ++i)
            BPE_REQUIRE(cuts[i] >= cuts[i - 1], BPE_E_ARG, "chunk starts must be sorted");
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : tok->stream;
        *n_out = bpe::encode_device(*tok, d_utf8, n, d_out, s, cuts);
    });
}

int bpe_tok_encode_file_u16(bpe_tokenizer* tok, const char* path, size_t chars_per_piece, uint16_t* ids_out,
                            size_t cap, size_t* n_out, double* phase_ms) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && path && n_out && chars_per_piece > 0, BPE_E_ARG, "NULL argument");
        *n_out = 0;
        double ph[4] = {0, 0, 0, 0};
        const bpe::Source src = bpe::Source::open_path(path);   // FileNotFoundError etc. before the GPU
        int dev = 0;
        BPE_HIP(hipGetDevice(&dev));
        const size_t k = bpe::encode_file_pipelined(*tok, src, chars_per_piece, ids_out, cap, dev, ph);
        *n_out = k;
        if (phase_ms) std::memcpy(phase_ms, ph, sizeof(ph));
    });
}

int bpe_tok_encode_files(bpe_tokenizer* tok, const char* const* paths, size_t n_paths, const char* out_path,
                         const bpe_dataset_opts* opts, uint64_t* file_id_offsets, uint64_t* id_counts,
                         size_t n_counts, bpe_dataset_stats* stats) {
    // the outputs under temporary names beside their paths: renamed after success, removed after an error
    struct TmpFile {
        std::string path, tmp;
        int fd = -1;
        void open(const char* p) {
            path = p;
            tmp = path + ".tmp" + std::to_string((long long)::getpid());
            fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
            if (fd < 0) throw bpe::Error{BPE_E_IO, "cannot create " + tmp, errno};
        }
        void commit() {
            const int rc = ::close(fd);
            fd = -1;
            if (rc != 0 || ::rename(tmp.c_str(), path.c_str()) != 0)
                throw bpe::Error{BPE_E_IO, "cannot write " + path, errno};
            tmp.clear();
        }
        ~TmpFile() {
            if (fd >= 0) ::close(fd);
            if (!tmp.empty()) ::unlink(tmp.c_str());
        }
    };
    try {
        BPE_REQUIRE(tok && out_path && opts && (n_paths == 0 || paths), BPE_E_ARG, "NULL argument");
        const bpe_dataset_opts& O = *opts;
        BPE_REQUIRE(O.chars_per_piece > 0, BPE_E_ARG, "chars_per_piece must be positive");
        BPE_REQUIRE(O.window_bytes == 0 || O.window_bytes >= 65536, BPE_E_ARG, "window_bytes must be at least 65536");
        BPE_REQUIRE(O.id_bytes == 2 || O.id_bytes == 4, BPE_E_ARG, "id_bytes must be 2 or 4");
        BPE_REQUIRE((O.has_separator != 0) == (O.index_path != nullptr), BPE_E_ARG,
                    "a separator needs an index path, and an index path a separator");
        BPE_REQUIRE(!id_counts || (n_counts > 0 && n_counts <= (1ull << 32)), BPE_E_ARG, "bad id table size");
        for (size_t i = 0; i < n_paths; ++i) BPE_REQUIRE(paths[i], BPE_E_ARG, "NULL path");
        bpe_dataset_stats st{};
        tok->fix_total = bpe_utf8_stats{0, 0, ~0ULL};
        tok->fix_first_file = 0;
        tok->fix_file_units.assign(n_paths, 0);
        if (file_id_offsets) std::fill(file_id_offsets, file_id_offsets + n_paths + 1, (uint64_t)0);
        if (id_counts) std::fill(id_counts, id_counts + n_counts, (uint64_t)0);
        TmpFile out, idx;
        out.open(out_path);
        if (O.index_path) idx.open(O.index_path);
        if (n_paths) {
            int dev = 0;
            BPE_HIP(hipGetDevice(&dev));
            if (O.id_bytes == 2)
                bpe::encode_files_pipelined<uint16_t>(*tok, paths, n_paths, out.fd, idx.fd, O, file_id_offsets,
                                                      id_counts, n_counts, st, dev);
            else
                bpe::encode_files_pipelined<uint32_t>(*tok, paths, n_paths, out.fd, idx.fd, O, file_id_offsets,
                                                      id_counts, n_counts, st, dev);
        }
        if (O.index_path) idx.commit();
        out.commit();
        if (stats) *stats = st;
        bpe::set_error(0, "");
        return BPE_OK;
    } catch (const bpe::Error& e) {
        bpe::set_error(e.code, e.msg, e.sys_errno);
        return e.code;
    } catch (const std::bad_alloc&) {
        bpe::set_error(BPE_E_NOMEM, "host allocation failed");
        return BPE_E_NOMEM;
    }
}

int bpe_tok_set_errors(bpe_tokenizer* tok, int mode) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok, BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(mode >= BPE_UTF8_STRICT && mode <= BPE_UTF8_IGNORE, BPE_E_ARG,
                    "mode must be 0 (strict), 1 (replace) or 2 (ignore)");
        tok->errors = mode;
    });
}

int bpe_tok_utf8_report(const bpe_tokenizer* tok, bpe_utf8_stats* total, uint64_t* first_file, uint64_t* file_units,
                        size_t n_files) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && (n_files == 0 || file_units), BPE_E_ARG, "NULL argument");
        if (total) *total = tok->fix_total;
        if (first_file) *first_file = tok->fix_first_file;
        for (size_t i = 0; i < n_files; ++i) file_units[i] = i < tok->fix_file_units.size() ? tok->fix_file_units[i] : 0;
    });
}

int bpe_tok_encode_chunks(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* starts,
                          size_t n_starts, uint32_t* ids_out, size_t cap, size_t* n_out) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && (n == 0 || (utf8 && ids_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(cap >= n, BPE_E_ARG, "ids_out capacity must be >= input bytes");
        BPE_REQUIRE(n_starts == 0 || starts, BPE_E_ARG, "NULL starts");
        *n_out = 0;
        if (n == 0) return;
        std::vector<unsigned long long> cuts(starts, starts + n_starts);
        for (size_t i = 1; i < cuts.size(); ++i)
            BPE_REQUIRE(cuts[i] >= cuts[i - 1], BPE_E_ARG, "chunk starts must be sorted");
        bpe::DevBuf<uint8_t> d_text(n);
        bpe::DevBuf<uint32_t> d_out(n);
        BPE_HIP(hipMemcpyAsync(d_text.p, utf8, n, hipMemcpyHostToDevice, tok->stream));
        const size_t m = bpe::encode_device(*tok, d_text.p, n, d_out.p, tok->stream, cuts);
        if (m) BPE_HIP(hipMemcpyAsync(ids_out, d_out.p, m * 4, hipMemcpyDeviceToHost, tok->stream));
        BPE_HIP(hipStreamSynchronize(tok->stream));
        *n_out = m;
    });
}

int bpe_tok_encode_batch_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                size_t n_docs, uint32_t* d_out, size_t* n_out, uint64_t* d_id_offsets, void* hip_stream) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && d_id_offsets && (n == 0 || (d_utf8 && d_out)), BPE_E_ARG, "NULL argument");
        const std::vector<unsigned long long> cuts = bpe::batch_cuts(doc_starts, n_docs, n);
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : tok->stream;
        *n_out = 0;
        if (n == 0) {   // empty documents only: every offset is 0
            BPE_HIP(hipMemsetAsync(d_id_offsets, 0, (n_docs + 1) * sizeof(uint64_t), s));
            BPE_HIP(hipStreamSynchronize(s));
            return;
        }
        const bpe::DocStarts docs{doc_starts, n_docs, reinterpret_cast<unsigned long long*>(d_id_offsets)};
        *n_out = bpe::encode_device(*tok, d_utf8, n, d_out, s, cuts, &docs);
    });
}

int bpe_tok_encode_batch(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts,
                         size_t n_docs, uint32_t* ids_out, size_t cap, size_t* n_out, uint64_t* id_offsets_out) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && id_offsets_out && (n == 0 || (utf8 && ids_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(cap >= n, BPE_E_ARG, "ids_out capacity must be >= input bytes");
        const std::vector<unsigned long long> cuts = bpe::batch_cuts(doc_starts, n_docs, n);
        *n_out = 0;
        if (n == 0) {
            std::fill(id_offsets_out, id_offsets_out + n_docs + 1, (uint64_t)0);
            return;
        }
        bpe::DevBuf<uint8_t> d_text(n);
        bpe::DevBuf<uint32_t> d_out(n);
        bpe::DevBuf<unsigned long long> d_off(n_docs + 1);
        BPE_HIP(hipMemcpyAsync(d_text.p, utf8, n, hipMemcpyHostToDevice, tok->stream));
        const bpe::DocStarts docs{doc_starts, n_docs, d_off.p};
        const size_t m = bpe::encode_device(*tok, d_text.p, n, d_out.p, tok->stream, cuts, &docs);
        if (m) BPE_HIP(hipMemcpyAsync(ids_out, d_out.p, m * 4, hipMemcpyDeviceToHost, tok->stream));
        BPE_HIP(hipMemcpyAsync(id_offsets_out, d_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, tok->stream));
        BPE_HIP(hipStreamSynchronize(tok->stream));
        *n_out = m;
    });
}

int bpe_tok_encode_spans_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                size_t n_docs, int unit, uint32_t* d_ids, size_t* n_out, uint64_t* d_id_offsets,
                                uint32_t* d_spans, void* hip_stream) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && d_id_offsets && (n == 0 || (d_utf8 && d_ids && d_spans)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(unit == 0 || unit == 1, BPE_E_ARG, "unit must be 0 (byte) or 1 (char)");
        BPE_REQUIRE((reinterpret_cast<uintptr_t>(d_spans) & 7u) == 0, BPE_E_ARG, "d_spans must be 8-byte aligned");
        BPE_REQUIRE(!tok->span_shared, BPE_E_ARG,
                    "spans are not defined for this vocab: one id names byte strings of different lengths");
        const std::vector<unsigned long long> cuts = bpe::batch_cuts(doc_starts, n_docs, n);
        for (size_t i = 0; i < n_docs; ++i)
            BPE_REQUIRE(((i + 1 < n_docs ? doc_starts[i + 1] : (uint64_t)n) - doc_starts[i]) >> 32 == 0, BPE_E_LIMIT,
                        "a document of 2^32 bytes or more: its spans do not fit uint32");
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : tok->stream;
        *n_out = 0;
        if (n == 0) {   // empty documents only: every offset is 0, no span
            BPE_HIP(hipMemsetAsync(d_id_offsets, 0, (n_docs + 1) * sizeof(uint64_t), s));
            BPE_HIP(hipStreamSynchronize(s));
            return;
        }
        const bpe::DocStarts docs{doc_starts, n_docs, reinterpret_cast<unsigned long long*>(d_id_offsets)};
        const bpe::SpanOut so{reinterpret_cast<uint2*>(d_spans), unit};
        *n_out = bpe::encode_device(*tok, d_utf8, n, d_ids, s, cuts, &docs, &so);
    });
}

int bpe_tok_encode_spans(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts, size_t n_docs,
                         int unit, uint32_t* ids_out, size_t cap, size_t* n_out, uint64_t* id_offsets_out,
                         uint32_t* spans_out, size_t spans_cap) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && id_offsets_out && (n == 0 || (utf8 && ids_out && spans_out)), BPE_E_ARG,
                    "NULL argument");
        BPE_REQUIRE(cap >= n && spans_cap >= n, BPE_E_ARG, "ids_out and spans_out capacities must be >= input bytes");
        BPE_REQUIRE(unit == 0 || unit == 1, BPE_E_ARG, "unit must be 0 (byte) or 1 (char)");
        *n_out = 0;
        bpe::DevBuf<uint8_t> d_text(n);
        bpe::DevBuf<uint32_t> d_out(n);
        bpe::DevBuf<uint2> d_spans(n);
        bpe::DevBuf<unsigned long long> d_off(n_docs + 1);
        if (n) BPE_HIP(hipMemcpyAsync(d_text.p, utf8, n, hipMemcpyHostToDevice, tok->stream));
        size_t m = 0;
        const int rc = bpe_tok_encode_spans_device(tok, d_text.p, n, doc_starts, n_docs, unit, d_out.p, &m,
                                                   reinterpret_cast<uint64_t*>(d_off.p),
                                                   reinterpret_cast<uint32_t*>(d_spans.p), tok->stream);
        if (rc != BPE_OK) throw bpe::Error{rc, bpe_last_error()};
        if (m) {
            BPE_HIP(hipMemcpyAsync(ids_out, d_out.p, m * 4, hipMemcpyDeviceToHost, tok->stream));
            BPE_HIP(hipMemcpyAsync(spans_out, d_spans.p, m * 8, hipMemcpyDeviceToHost, tok->stream));
        }
        BPE_HIP(hipMemcpyAsync(id_offsets_out, d_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, tok->stream));
        BPE_HIP(hipStreamSynchronize(tok->stream));
        *n_out = m;
    });
}

int bpe_ids_pack_rows_device(const uint32_t* d_ids, const uint64_t* d_offsets, size_t n_rows, size_t row_len,
                             int64_t pad, int flags, int elem_bytes, void* d_out, int32_t* d_lengths,
                             void* hip_stream) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(elem_bytes == 4 || elem_bytes == 8, BPE_E_ARG, "elem_bytes must be 4 or 8");
        BPE_REQUIRE((flags & ~(bpe::kPackKeepLast | bpe::kPackPadLeft)) == 0, BPE_E_ARG, "unknown flags");
        BPE_REQUIRE(elem_bytes == 8 || (pad >= INT32_MIN && pad <= INT32_MAX), BPE_E_ARG, "pad does not fit int32");
        BPE_REQUIRE(row_len <= (size_t)INT32_MAX, BPE_E_ARG, "row_len does not fit the int32 lengths");
        if (n_rows == 0) return;
        BPE_REQUIRE(d_offsets && d_lengths && (row_len == 0 || d_out), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(row_len == 0 || n_rows <= SIZE_MAX / 8 / row_len, BPE_E_ARG, "n_rows x row_len overflows");
        hipStream_t s = (hipStream_t)hip_stream;
        const size_t per = 16 / (size_t)elem_bytes;
        const bool vec = row_len % per == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0;
        const unsigned grid = bpe::grid_for(std::max(n_rows, n_rows * row_len / (vec ? per : 1)), 256);
        const unsigned long long* off = reinterpret_cast<const unsigned long long*>(d_offsets);
        if (elem_bytes == 4) {
            bpe::DevBuf<unsigned> over(2);   // {an id >= 2^31 was kept, the smallest such id}
            const unsigned init[2] = {0u, 0xffffffffu};
            unsigned got[2] = {0u, 0u};
            BPE_HIP(hipMemcpyAsync(over.p, init, sizeof(init), hipMemcpyHostToDevice, s));
            auto k = vec ? bpe::k_pack_rows<int32_t, true> : bpe::k_pack_rows<int32_t, false>;
            hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, d_ids, off, n_rows, row_len, (int32_t)pad, flags,
                               static_cast<int32_t*>(d_out), d_lengths, over.p);
            BPE_HIP(hipGetLastError());
            BPE_HIP(hipMemcpyAsync(got, over.p, sizeof(got), hipMemcpyDeviceToHost, s));
            BPE_HIP(hipStreamSynchronize(s));
            BPE_REQUIRE(!got[0], BPE_E_LIMIT, "token id " + std::to_string(got[1]) +
                                                  " does not fit int32 rows (ids from 2^31 on need elem_bytes 8)");
            return;
        }
        auto k = vec ? bpe::k_pack_rows<int64_t, true> : bpe::k_pack_rows<int64_t, false>;
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, s, d_ids, off, n_rows, row_len, pad, flags,
                           static_cast<int64_t*>(d_out), d_lengths, static_cast<unsigned*>(nullptr));
        BPE_HIP(hipGetLastError());
        BPE_HIP(hipStreamSynchronize(s));
    });
}

int bpe_tok_encode_gpus(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, uint32_t* ids_out, size_t cap,
                        size_t* n_out, int n_gpus) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok && n_out && (n == 0 || (utf8 && ids_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(cap >= n, BPE_E_ARG, "ids_out capacity must be >= input bytes");
        *n_out = 0;
        if (n == 0) return;
        *n_out = bpe::encode_gpus(*tok, utf8, n, ids_out, n_gpus);
    });
}

int bpe_tok_release_buffers(bpe_tokenizer* tok) {
    return bpe::guarded_enc([&] {
        BPE_REQUIRE(tok, BPE_E_ARG, "NULL argument");
        BPE_HIP(hipStreamSynchronize(tok->stream));
        tok->recs_cache = bpe::DevBuf<uint32_t>();
        tok->sc = bpe_tokenizer::Scratch();
        std::lock_guard<std::mutex> g(tok->copies_m);
        tok->copies.clear();
    });
}

void bpe_tok_free(bpe_tokenizer* tok) { delete tok; }

}  // extern "C"
