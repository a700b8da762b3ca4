// Merge loop, device state: the round state, the pair table, token and posting-index
// structures, candidates and their order, pair-table and token helpers.
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include <climits>
#include <cstddef>

#include "internal.h"
#include "prims.h"

namespace bpe {

namespace {

constexpr unsigned kPresent = 1u, kInC = 2u;
enum : int { HALT_NONE = 0, HALT_REBUILD = 1, HALT_DONE = 2, HALT_HOST = 3 };
enum : unsigned { ERR_PAIRS_FULL = 1u, ERR_C_FULL = 2u, ERR_POOL = 4u };
constexpr unsigned long long kPolyP = 0x100000001B3ULL * 0x9E3779B97F4A7C15ULL | 1ULL;
constexpr int kNumCls = 4;
constexpr int kHistReplicas = 16;

struct RoundState {
    int halt;
    int round;
    int n_rounds;
    int ntok;
    long long T;
    unsigned nC, capC, c_limit, probe_merge_done;   // probe_*_done: BPE355_PROBE workgroup counters
    unsigned nC_base;           // |C| before this round's appends (set by k_merge)
    int cur_round, cur_ntok;    // for k_apply_argmax: this round, and ntok after it (k_merge)
    unsigned cur_a, cur_b, cur_new, cur_slot;
    long long cur_cnt;
    int new_is_new;
    unsigned err;
    unsigned n_single;
    unsigned n_single_new;      // batched: words the current trip's rewrite made single (the apply folds
                                // them into n_single, which the trip's own select phase reads)
    unsigned pool_used, pool_cap;
    unsigned long long pair_used;
    unsigned long long scan_slots;
    int nparts;                 // batched: apply workgroups whose top-M lists part[] holds
    unsigned probe_apply_done;
    unsigned long long* probe;  // BPE355_PROBE: phase stamps of sampled trips (else null)
    // batched rounds (k_select): the host's limits, checked before every trip
    int host_round;             // hand back to the host at this round (compaction schedule)
    unsigned single_limit;      // ... or when this many words became one token (compaction)
    unsigned max_len;           // longest word (bytes): the most one new token adds to the pool
    int max_batch;              // merges allowed per trip (1: one merge per trip)
    unsigned long long pair_limit;   // ... or when the pair table could pass this many keys
    long long narrow_limit;     // the merge sums a member's cells in 32-bit LDS words while count(P1) is
                                // below this: 2^32 (a cell never exceeds count(P_j) <= count(P1)), 0 under
                                // the test knob BPE355_LDS_CELLS=0 (every cell to the global 64-bit atomics)
};

struct Partial {
    long long cnt;
    unsigned long long ka, kb;   // key8 of a and of b (first 8 bytes, big-endian)
    unsigned slot, a, b, pad;
};

struct PairsDev {
    unsigned long long* key;  // ((a << 32) | b) + 1, 0 = empty
    long long* cnt;
    unsigned* flag;           // kPresent | kInC
    size_t mask;
    uint4* C;                 // candidate list: {slot, a, b, 0} (ids carried so the argmax loads
                              // the slot's count and the tokens' prefixes in one step)
};

struct ToksDev {
    uint8_t* pool;
    uint32_t* off;
    uint32_t* len;
    unsigned long long* hash;  // polynomial hash of the bytes
    unsigned long long* pw;    // P^len
    unsigned long long* key8;  // first 8 bytes, big-endian, zero padded
    unsigned long long* map;   // token dedupe map: (hash >> 32) << 32 | id + 1 (map_entry)
    uint32_t map_mask;
};

__host__ __device__ constexpr int slot_w(int c) { return 8 << c; }   // 8, 16, 32, 64 ids
__host__ __device__ inline int class_for(unsigned len) {
    return len <= 7 ? 0 : len <= 15 ? 1 : len <= 31 ? 2 : len <= 63 ? 3 : kNumCls;
}

template <class TokT>
struct SlotCls {
    TokT* slot;                  // n * slot_w(c) ids
    unsigned long long* cnt;
    unsigned n, blk0, nblk, pad;
};

template <class TokT>
struct WordsDev {
    SlotCls<TokT> c[kNumCls];
    TokT* ltok;                  // long words (> 63 ids): CSR
    unsigned long long* lbeg;
    uint32_t* llen;
    unsigned long long* lcnt;
    unsigned ln, lblk0, lnblk, pad;
    unsigned off[kNumCls + 1];   // flat word index: class c holds [off[c], off[c+1])
};

// Posting index over the slot words, rebuilt at every compaction: list[beg[t], beg[t]+len[t])
// holds the flat index of every word that contained token t at build time.  A token created
// later gets (beg, len) of the smaller covering list of its two parts (a word that contains it
// contained both parts when it was formed) -- stored per token, so the merge kernel finds its
// list in one dependent load; a token re-created through token dedupe (its bytes reached by
// another split) is marked uncovered (len = kNoAnc) until the next build.
constexpr unsigned kNoAnc = 0xffffffffu;
struct IndexDev {
    const uint32_t* list;
    uint32_t* beg;
    uint32_t* len;
    unsigned full_threshold;   // lists longer than this are cheaper to replace by a full scan
    unsigned n_slot_words;
};

template <class TokT> __host__ __device__ constexpr TokT sentinel() { return (TokT)~(TokT)0; }

// bytes(x) vs bytes(y) for tokens whose 8-byte prefixes are equal: -1 / 0 / +1
__device__ __forceinline__ int cmp_tok_tail(const uint8_t* __restrict__ pool, const uint32_t* __restrict__ off,
                                         const uint32_t* __restrict__ len, unsigned x, unsigned y) {
    const unsigned lx = len[x], ly = len[y], m = lx < ly ? lx : ly;
    const uint8_t* px = pool + off[x];
    const uint8_t* py = pool + off[y];
    for (unsigned i = 8; i < m; ++i)
        if (px[i] != py[i]) return px[i] < py[i] ? -1 : 1;
    return lx < ly ? -1 : (lx > ly ? 1 : 0);
}

// The reference's max key (count, bytes a, bytes b) (train.py:187-189).  Byte strings compare
// by their zero-padded big-endian 8-byte prefix first: a smaller prefix means smaller bytes;
// only equal prefixes of different tokens need the bytes themselves (rare: long tokens, or a
// prefix relation like "ab" vs "ab\0").
struct Cand {
    long long cnt;
    unsigned long long ka, kb;
    unsigned slot, a, b;
};
__device__ __forceinline__ bool cand_better(const Cand& x, const Cand& y, const uint8_t* pool,
                                            const uint32_t* off, const uint32_t* len) {
    if (x.cnt != y.cnt) return x.cnt > y.cnt;
    if (x.a != y.a) {
        if (x.ka != y.ka) return x.ka > y.ka;
        return cmp_tok_tail(pool, off, len, x.a, y.a) > 0;
    }
    if (x.b != y.b) {
        if (x.kb != y.kb) return x.kb > y.kb;
        return cmp_tok_tail(pool, off, len, x.b, y.b) > 0;
    }
    return false;
}
__device__ __forceinline__ Cand cand_none() { return Cand{LLONG_MIN, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ Cand shfl_xor_cand(const Cand& c, int o) {
    Cand r;
    r.cnt = __shfl_xor(c.cnt, o);
    r.ka = __shfl_xor(c.ka, o);
    r.kb = __shfl_xor(c.kb, o);
    r.slot = __shfl_xor(c.slot, o);
    r.a = __shfl_xor(c.a, o);
    r.b = __shfl_xor(c.b, o);
    return r;
}


// ------------------------------------------------------------------ pair table
// returns the slot of key (inserting it if absent, *inserted = 1), or ~0 if the table is full
__device__ __forceinline__ size_t pair_slot(const PairsDev& P, unsigned long long key,
                                            RoundState* st, bool* inserted) {
    size_t s = mix64(key) & P.mask;
    *inserted = false;
    for (size_t probe = 0; probe <= P.mask; ++probe) {
        unsigned long long k = P.key[s];
        if (k == key) return s;
        if (k == 0) {
            k = atomicCAS(&P.key[s], 0ULL, key);
            if (k == 0) {
                atomicAdd(&st->pair_used, 1ULL);
                *inserted = true;
                return s;
            }
            if (k == key) return s;
        }
        s = (s + 1) & P.mask;
    }
    atomicOr(&st->err, ERR_PAIRS_FULL);
    return ~(size_t)0;
}

__device__ __forceinline__ unsigned long long pair_key(unsigned p, unsigned q) {
    return ((((unsigned long long)p) << 32) | q) + 1ULL;
}

// frequencies[(p, q)] -= d  (a missing key would be created, as defaultdict does)
__device__ __forceinline__ void pair_dec(const PairsDev& P, RoundState* st, unsigned p, unsigned q,
                                         long long d) {
    bool ins;
    const size_t s = pair_slot(P, pair_key(p, q), st, &ins);
    if (s == ~(size_t)0) return;
    atomicAdd((unsigned long long*)&P.cnt[s], (unsigned long long)(-d));
    if (ins) atomicOr(&P.flag[s], kPresent);
}

// frequencies[(p, q)] += d; the key is present from now on.  Returns the slot so the caller
// can list it as touched: whether it enters the candidate list is decided from its FINAL
// count in k_argmax -- never from the order the atomics happened to land in, which differs
// between ranks and would let replicated pair tables disagree about C.
__device__ __forceinline__ size_t pair_inc(const PairsDev& P, RoundState* st, unsigned p, unsigned q,
                                           long long d) {
    bool ins;
    const size_t s = pair_slot(P, pair_key(p, q), st, &ins);
    if (s == ~(size_t)0) return s;
    atomicAdd((unsigned long long*)&P.cnt[s], (unsigned long long)d);
    atomicOr(&P.flag[s], kPresent);
    return s;
}

// ------------------------------------------------------------------ token helpers
__device__ __forceinline__ unsigned long long concat_key8(const ToksDev& K, unsigned a, unsigned b) {
    const unsigned la = K.len[a];
    const unsigned long long ka = K.key8[a];
    if (la >= 8) return ka;
    return ka | (K.key8[b] >> (8 * la));
}

__device__ __forceinline__ uint8_t concat_byte(const ToksDev& K, unsigned a, unsigned la,
                                               unsigned b, unsigned i) {
    return i < la ? K.pool[K.off[a] + i] : K.pool[K.off[b] + (i - la)];
}

__device__ bool equals_concat(const ToksDev& K, unsigned x, unsigned a, unsigned b) {
    const unsigned la = K.len[a], ln = la + K.len[b];
    if (K.len[x] != ln) return false;
    const uint8_t* px = K.pool + K.off[x];
    for (unsigned i = 0; i < ln; ++i)
        if (px[i] != concat_byte(K, a, la, b, i)) return false;
    return true;
}

// The token dedupe map (vocab.py:29: a merge whose bytes exist reuses that id): open addressing
// on mix64(hash), entries tagged with the hash's high half, so a probe that meets another token
// moves on without loading that token's hash
__device__ __forceinline__ unsigned long long map_entry(unsigned long long h, unsigned id) {
    return (h & 0xffffffff00000000ull) | (unsigned long long)(id + 1);
}
// the id of the token whose bytes are a + b (hash h, ln bytes), or ~0
__device__ __forceinline__ unsigned map_find(const ToksDev& K, unsigned long long h, unsigned ln, unsigned a,
                                             unsigned b) {
    unsigned s = (unsigned)mix64(h) & K.map_mask;
    for (unsigned long long e = K.map[s]; e != 0; s = (s + 1) & K.map_mask, e = K.map[s]) {
        if ((e >> 32) != (h >> 32)) continue;
        const unsigned id = (unsigned)e - 1;
        if (K.hash[id] == h && K.len[id] == ln && equals_concat(K, id, a, b)) return id;
    }
    return ~0u;
}

}  // namespace

}  // namespace bpe
