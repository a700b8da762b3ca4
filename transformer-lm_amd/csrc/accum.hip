// The word accumulator: a device-resident word table that owns its bytes and sums counts over
// many inputs (files, windows of a file, pre-counted words, other accumulators).
//
// Why training on it is exact: the reference's trainer (models/tokenizer/train.py:16-49) sees the
// corpus only through the multiset {pre-token -> count} (the argument is written out at the top of
// exchange.hip).  Every input is pre-tokenized on its own, exactly as a separate
// extract_subword_frequencies call on it would, and the accumulator holds the word-by-word sum of
// those multisets; the merge loop then runs on that table as it runs on a corpus's own.
//
// Layout: the open-addressing {key, count} + pos table of stage.h over an append-only byte pool.
// A word of <= 7 bytes has the inline key (kInl | len << 56 | bytes) and pos[slot] = its pool
// offset; a longer one has key = len << 40 | pool offset + 1.  So MergeLoop(stream, nullptr, pool,
// ...).build_words(table, specials) reads it as it reads a corpus's table.
//
// Fold (a shard's table, host records or another accumulator into this one), in two launches
// around one size read-back, so that the pool holds no byte of a duplicate:
//   1. k_fold_lookup: one thread per incoming word looks it up.  Nothing is inserted in this
//      launch, so the keys are stable: a hit adds its count with one atomic, a miss is appended
//      (one atomic per wave) to the list of new words.
//   2. the new words' lengths are scanned into pool offsets; the host grows the table (rehash
//      into twice the slots, before the load passes 1/2) and the pool (geometrically) if needed.
//   3. k_fold_insert: one thread per new word copies its bytes into the pool and claims an empty
//      slot with a compare-and-swap (table_add's discipline).  The incoming words are distinct
//      (a shard's table is unique; host records are deduplicated before the upload) and none is
//      in the table, so an occupied slot is never the same word: probe on without a compare.
// All device arrays of a fold are grow-only members: no allocation or free per fold once they
// have reached their size (a freed device buffer synchronises the device).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "internal.h"
#include "prims.h"
#include "stage.h"

namespace bpe {

namespace {

constexpr size_t kMissSlot = ~(size_t)0, kFullSlot = ~(size_t)0 - 1;
constexpr unsigned long long kPoolLimit = kOffMask - 1;   // offset + 1 must fit 40 bits
constexpr uint64_t kWeightLimit = 1ULL << 62;
constexpr size_t kPoolPad = 16;

// the word a key names: its length and where its bytes lie in the table's text
__device__ __forceinline__ void key_word(unsigned long long k, const unsigned long long* __restrict__ pos, size_t slot,
                                         uint32_t& len, unsigned long long& off) {
    const bool inl = (k >> 63) != 0;
    len = inl ? (uint32_t)((k >> 56) & 0x7f) : (uint32_t)(k >> 40);
    off = inl ? pos[slot] : (k & kOffMask) - 1;
}

// a word's hash as the tables take it: packed bytes up to kInline, else hash_word
__device__ __forceinline__ uint64_t word_hash(const uint8_t* __restrict__ t, size_t p, size_t len, uint64_t& wl,
                                              uint64_t& wh) {
    wl = 0;
    wh = 0;
    if (len <= (size_t)kInline) {
        pack_word(t, p, len, wl, wh);
        return short_hash(wl, wh, len);
    }
    return hash_word(t, p, len);
}

// the slot of the word t[p, p + len) in a table over `pool` whose keys do not change during the
// launch; kMissSlot: not there, kFullSlot: probe limit
__device__ __forceinline__ size_t acc_find(const uint8_t* __restrict__ pool, const unsigned long long* __restrict__ kv,
                                           size_t mask, const uint8_t* __restrict__ t, size_t p, size_t len,
                                           uint64_t wl, uint64_t wh, uint64_t h) {
    const bool inl = len <= (size_t)kInlineKey;
    const unsigned long long mine = kInl | ((unsigned long long)len << 56) | wl;
    size_t slot = h & mask;
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        const unsigned long long k = kv[2 * slot];
        if (k == 0) return kMissSlot;
        bool eq = false;
        if (inl) {
            eq = k == mine;
        } else if (!(k & kInl) && (k >> 40) == len) {
            const size_t q = (k & kOffMask) - 1;
            if (len <= (size_t)kInline) {
                uint64_t l2, h2;
                pack_word(pool, q, len, l2, h2);
                eq = l2 == wl && h2 == wh;
            } else {
                eq = words_equal(pool, q, t, p, len);
            }
        }
        if (eq) return slot;
        slot = (slot + 1) & mask;
    }
    return kFullSlot;
}

// claim an empty slot for a key that is in the table nowhere; ~0: probe limit (status bit 1)
__device__ __forceinline__ size_t acc_claim(unsigned long long* __restrict__ kv, size_t mask, uint64_t h,
                                            unsigned long long mine, unsigned* __restrict__ status) {
    size_t slot = h & mask;
    for (int probe = 0; probe < kMaxProbe; ++probe) {
        if (kv[2 * slot] == 0 && atomicCAS(&kv[2 * slot], 0ULL, mine) == 0) return slot;
        slot = (slot + 1) & mask;
    }
    atomicOr(status, 1u);
    return ~(size_t)0;
}

__global__ void __launch_bounds__(256) k_occupied(const unsigned long long* __restrict__ kv, size_t cap,
                                                  unsigned long long* __restrict__ n) {
    unsigned mine = 0;
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < cap; s += (size_t)gridDim.x * 256)
        mine += kv[2 * s] != 0;
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n, (unsigned long long)mine);
}

// occupied slots of a table over `text` -> (offset, length, count) records; words equal to a
// special are left out (train.py:25)
__global__ void __launch_bounds__(256) k_list_table(const unsigned long long* __restrict__ kv,
                                                    const unsigned long long* __restrict__ pos, size_t cap,
                                                    const uint8_t* __restrict__ text, const uint8_t* __restrict__ sp_bytes,
                                                    const uint32_t* __restrict__ sp_off,
                                                    const uint32_t* __restrict__ sp_len, int n_sp,
                                                    unsigned long long* __restrict__ w_off, uint32_t* __restrict__ w_len,
                                                    unsigned long long* __restrict__ w_cnt, unsigned* __restrict__ n_out,
                                                    unsigned cap_out) {
    // (every lane of a wave runs every trip: wave_append needs them all)
    for (size_t base = (size_t)blockIdx.x * 256; base < cap; base += (size_t)gridDim.x * 256) {
        const size_t s = base + threadIdx.x;
        const unsigned long long k = s < cap ? kv[2 * s] : 0ULL;
        bool keep = k != 0;
        uint32_t len = 0;
        unsigned long long off = 0;
        if (keep) key_word(k, pos, s, len, off);
        for (int i = 0; keep && i < n_sp; ++i) {
            if (sp_len[i] != len) continue;
            bool eq = true;
            for (uint32_t j = 0; j < len && eq; ++j) eq = text[off + j] == sp_bytes[sp_off[i] + j];
            if (eq) keep = false;
        }
        const unsigned idx = wave_append(keep, n_out);
        if (!keep || idx >= cap_out) continue;
        w_off[idx] = off;
        w_len[idx] = len;
        w_cnt[idx] = kv[2 * s + 1];
    }
}

// step 1 of a fold: hits add their counts, misses are listed.  cnts: [0] new words, [1] status
__global__ void __launch_bounds__(256) k_fold_lookup(const uint8_t* __restrict__ text,
                                                     const unsigned long long* __restrict__ w_off,
                                                     const uint32_t* __restrict__ w_len,
                                                     const unsigned long long* __restrict__ w_cnt, size_t n,
                                                     const uint8_t* __restrict__ pool, unsigned long long* __restrict__ kv,
                                                     size_t mask, unsigned long long* __restrict__ w_hash,
                                                     unsigned* __restrict__ new_idx, unsigned* __restrict__ cnts) {
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        const size_t i = base + threadIdx.x;
        bool miss = false;
        if (i < n) {
            const size_t len = w_len[i], p = w_off[i];
            if (len >= kMaxPretok) {
                atomicOr(&cnts[1], 2u);
            } else {
                uint64_t wl, wh;
                const uint64_t h = word_hash(text, p, len, wl, wh);
                w_hash[i] = h;
                const size_t slot = acc_find(pool, kv, mask, text, p, len, wl, wh, h);
                if (slot == kFullSlot) atomicOr(&cnts[1], 1u);
                else if (slot == kMissSlot) miss = true;
                else atomicAdd(&kv[2 * slot + 1], w_cnt[i]);
            }
        }
        const unsigned j = wave_append(miss, &cnts[0]);
        if (miss) new_idx[j] = (unsigned)i;
    }
}

__global__ void k_new_lens(const uint32_t* __restrict__ w_len, const unsigned* __restrict__ new_idx, unsigned n_new,
                           unsigned long long* __restrict__ len64, unsigned long long extra) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_new) len64[j] = w_len[new_idx ? new_idx[j] : j] + extra;
}

// step 3 of a fold: each new word's bytes into the pool at pool_base + b_off[j], its key into
// an empty slot.  Nothing reads the pool or compares keys in this launch.
__global__ void __launch_bounds__(256) k_fold_insert(const uint8_t* __restrict__ text,
                                                     const unsigned long long* __restrict__ w_off,
                                                     const uint32_t* __restrict__ w_len,
                                                     const unsigned long long* __restrict__ w_cnt,
                                                     const unsigned long long* __restrict__ w_hash,
                                                     const unsigned* __restrict__ new_idx, unsigned n_new,
                                                     const unsigned long long* __restrict__ b_off,
                                                     unsigned long long pool_base, uint8_t* __restrict__ pool,
                                                     unsigned long long* __restrict__ kv,
                                                     unsigned long long* __restrict__ pos, size_t mask,
                                                     unsigned* __restrict__ cnts) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_new) return;
    const unsigned i = new_idx[j];
    const uint32_t len = w_len[i];
    const uint8_t* src = text + w_off[i];
    const unsigned long long at = pool_base + b_off[j];
    unsigned long long wl = 0;
    for (uint32_t b = 0; b < len; ++b) {
        const uint8_t v = src[b];
        pool[at + b] = v;
        if (b < (uint32_t)kInlineKey) wl |= (unsigned long long)v << (8 * b);
    }
    const unsigned long long mine = len <= (uint32_t)kInlineKey ? kInl | ((unsigned long long)len << 56) | wl
                                                                : ((unsigned long long)len << 40) | (at + 1);
    const size_t slot = acc_claim(kv, mask, w_hash[i], mine, &cnts[1]);
    if (slot == ~(size_t)0) return;
    pos[slot] = at;
    kv[2 * slot + 1] = w_cnt[i];   // (the slot was empty: its count is zero)
}

// every entry of the old table into the new one (twice the slots), over the same pool
__global__ void __launch_bounds__(256) k_rehash(const unsigned long long* __restrict__ okv,
                                                const unsigned long long* __restrict__ opos, size_t ocap,
                                                const uint8_t* __restrict__ pool, unsigned long long* __restrict__ kv,
                                                unsigned long long* __restrict__ pos, size_t mask,
                                                unsigned* __restrict__ cnts) {
    for (size_t s = (size_t)blockIdx.x * 256 + threadIdx.x; s < ocap; s += (size_t)gridDim.x * 256) {
        const unsigned long long k = okv[2 * s];
        if (!k) continue;
        uint32_t len;
        unsigned long long off;
        key_word(k, opos, s, len, off);
        uint64_t wl, wh;
        const uint64_t h = word_hash(pool, off, len, wl, wh);
        const size_t slot = acc_claim(kv, mask, h, k, &cnts[1]);
        if (slot == ~(size_t)0) continue;
        pos[slot] = opos[s];
        kv[2 * slot + 1] = okv[2 * s + 1];
    }
}

// listed words -> packed (u32 len, bytes, u64 count) records at b_off[i]
__global__ void __launch_bounds__(256) k_export_write(const uint8_t* __restrict__ pool,
                                                      const unsigned long long* __restrict__ w_off,
                                                      const uint32_t* __restrict__ w_len,
                                                      const unsigned long long* __restrict__ w_cnt,
                                                      const unsigned long long* __restrict__ b_off, unsigned n,
                                                      uint8_t* __restrict__ blob) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t len = w_len[i];
    const unsigned long long c = w_cnt[i];
    uint8_t* d = blob + b_off[i];
    for (int b = 0; b < 4; ++b) d[b] = (uint8_t)(len >> (8 * b));
    const uint8_t* src = pool + w_off[i];
    for (uint32_t b = 0; b < len; ++b) d[4 + b] = src[b];
    for (int b = 0; b < 8; ++b) d[4 + len + b] = (uint8_t)(c >> (8 * b));
}

size_t env_size(const char* name, size_t dflt, size_t lo) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    const long long v = std::atoll(e);
    return std::max(lo, (size_t)std::max(0LL, v));
}

struct DeviceScope {   // the accumulator's device for the duration of a call
    int prev = 0;
    explicit DeviceScope(int dev) {
        BPE_HIP(hipGetDevice(&prev));
        if (prev != dev) BPE_HIP(hipSetDevice(dev));
        else prev = -1;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

double ms_from(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

uint64_t sat_add(uint64_t a, uint64_t b) {
    uint64_t r;
    return __builtin_add_overflow(a, b, &r) ? ~0ULL : r;
}

}  // namespace

struct WordAccumulator::Scratch {
    DevBuf<unsigned long long> w_off, w_cnt, w_hash, b_off, len64, n_occ;
    DevBuf<uint32_t> w_len, sp_off, sp_len;
    DevBuf<unsigned> new_idx, cnts;
    DevBuf<uint8_t> tmp, seg, sp_bytes;
};

WordAccumulator::WordAccumulator() : sc_(std::make_unique<Scratch>()) {
    BPE_HIP(hipGetDevice(&dev_));
    BPE_HIP(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    try {
        const size_t cap = next_pow2(env_size("BPE355_ACC_SLOTS", (size_t)1 << 16, 16));
        pool_cap_ = env_size("BPE355_ACC_POOL", (size_t)1 << 20, 64);
        wc_.kv.alloc(2 * cap);
        wc_.pos.alloc(cap);
        wc_.cap = cap;
        pool_.alloc(pool_cap_ + kPoolPad);
        sc_->cnts.alloc(2);
        sc_->n_occ.alloc(1);
        BPE_HIP(hipMemsetAsync(wc_.kv.p, 0, wc_.kv.bytes(), s_));
        BPE_HIP(hipMemsetAsync(wc_.pos.p, 0, wc_.pos.bytes(), s_));
        BPE_HIP(hipStreamSynchronize(s_));
    } catch (...) {
        (void)hipStreamDestroy(s_);
        throw;
    }
}

WordAccumulator::~WordAccumulator() {
    if (s_) {
        (void)hipStreamSynchronize(s_);
        (void)hipStreamDestroy(s_);
    }
}

void WordAccumulator::clear() {
    DeviceScope ds(dev_);
    BPE_HIP(hipMemsetAsync(wc_.kv.p, 0, wc_.kv.bytes(), s_));
    BPE_HIP(hipMemsetAsync(wc_.pos.p, 0, wc_.pos.bytes(), s_));
    BPE_HIP(hipStreamSynchronize(s_));
    pool_used_ = 0;
    n_words_ = 0;
    shard_words_ = 0;
    weight_ = 0;
    wc_.n_pretokens = 0;
    st_ = AccumInfo{};
}

AccumInfo WordAccumulator::info() const {
    AccumInfo i = st_;
    i.n_words = n_words_;
    i.n_pretokens = wc_.n_pretokens;
    i.table_slots = wc_.cap;
    i.pool_bytes = pool_cap_;
    i.pool_live_bytes = pool_used_;
    return i;
}

void WordAccumulator::note_input(uint64_t n_bytes, uint64_t n_windows, uint64_t max_window, double load_ms,
                                 double count_ms) {
    st_.n_inputs += 1;
    st_.n_bytes += n_bytes;
    st_.n_windows += n_windows;
    st_.max_window_bytes = std::max(st_.max_window_bytes, max_window);
    st_.t_load_ms += load_ms;
    st_.t_count_ms += count_ms;
}

// Room for n_new more words and new_bytes more pool bytes: the table is rehashed into twice the
// slots (as often as needed, in one launch) before its load would pass 1/2, the pool at least
// doubles.  Both are rare by construction (geometric), so the allocation and the free they cost
// are not paid per fold.
void WordAccumulator::ensure(size_t n_new, size_t new_bytes) {
    BPE_REQUIRE(n_words_ + n_new < ((size_t)1 << 31), BPE_E_LIMIT, "more than 2^31 distinct words");
    BPE_REQUIRE(pool_used_ + new_bytes < kPoolLimit, BPE_E_LIMIT, "the word pool would pass 2^40 bytes");
    if (pool_used_ + new_bytes > pool_cap_) {
        const size_t cap = std::max(2 * pool_cap_, pool_used_ + new_bytes);
        DevBuf<uint8_t> np(cap + kPoolPad);
        if (pool_used_) BPE_HIP(hipMemcpyAsync(np.p, pool_.p, pool_used_, hipMemcpyDeviceToDevice, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        pool_ = std::move(np);
        pool_cap_ = cap;
        st_.n_grows += 1;
    }
    size_t cap = wc_.cap;
    while (2 * (n_words_ + n_new) > cap) cap *= 2;
    if (cap != wc_.cap) {
        DevBuf<unsigned long long> kv(2 * cap), pos(cap);
        BPE_HIP(hipMemsetAsync(kv.p, 0, kv.bytes(), s_));
        BPE_HIP(hipMemsetAsync(pos.p, 0, pos.bytes(), s_));
        BPE_HIP(hipMemsetAsync(sc_->cnts.p, 0, 8, s_));
        hipLaunchKernelGGL(k_rehash, dim3(grid_for(wc_.cap, 256)), dim3(256), 0, s_, wc_.kv.p, wc_.pos.p, wc_.cap,
                           pool_.p, kv.p, pos.p, cap - 1, sc_->cnts.p);
        BPE_HIP(hipGetLastError());
        unsigned h[2] = {0, 0};
        BPE_HIP(hipMemcpyAsync(h, sc_->cnts.p, 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        BPE_REQUIRE(!(h[1] & 1u), BPE_E_NOMEM, "accumulator rehash hit the probe limit");
        wc_.kv = std::move(kv);
        wc_.pos = std::move(pos);
        wc_.cap = cap;
        st_.n_grows += 1;
    }
}

void WordAccumulator::fold_list(const uint8_t* text, const unsigned long long* w_off, const uint32_t* w_len,
                                const unsigned long long* w_cnt, size_t n) {
    if (!n) return;
    Scratch& S = *sc_;
    BPE_REQUIRE(n < ((size_t)1 << 32), BPE_E_LIMIT, "more than 2^32 words in one fold");
    S.w_hash.reserve(n);
    S.new_idx.reserve(n);
    BPE_HIP(hipMemsetAsync(S.cnts.p, 0, 8, s_));
    hipLaunchKernelGGL(k_fold_lookup, dim3(grid_for(n, 256)), dim3(256), 0, s_, text, w_off, w_len, w_cnt, n,
                       pool_.p, wc_.kv.p, wc_.cap - 1, S.w_hash.p, S.new_idx.p, S.cnts.p);
    BPE_HIP(hipGetLastError());
    unsigned h[2] = {0, 0};
    BPE_HIP(hipMemcpyAsync(h, S.cnts.p, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    BPE_REQUIRE(!(h[1] & 2u), BPE_E_LIMIT, "a word of 8 MiB or more");
    BPE_REQUIRE(!(h[1] & 1u), BPE_E_NOMEM, "accumulator lookup hit the probe limit");
    const unsigned n_new = h[0];
    if (!n_new) return;
    S.len64.reserve(n_new);
    S.b_off.reserve(n_new);
    hipLaunchKernelGGL(k_new_lens, dim3(ceil_div(n_new, 256)), dim3(256), 0, s_, w_len, S.new_idx.p, n_new,
                       S.len64.p, 0ULL);
    exclusive_sum(S.len64.p, S.b_off.p, n_new, s_, &S.tmp);
    unsigned long long last[2];
    BPE_HIP(hipMemcpyAsync(&last[0], S.b_off.p + n_new - 1, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipMemcpyAsync(&last[1], S.len64.p + n_new - 1, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    const size_t new_bytes = (size_t)(last[0] + last[1]);
    ensure(n_new, new_bytes);
    BPE_HIP(hipMemsetAsync(S.cnts.p, 0, 8, s_));
    hipLaunchKernelGGL(k_fold_insert, dim3(ceil_div(n_new, 256)), dim3(256), 0, s_, text, w_off, w_len, w_cnt,
                       S.w_hash.p, S.new_idx.p, n_new, S.b_off.p, (unsigned long long)pool_used_, pool_.p, wc_.kv.p,
                       wc_.pos.p, wc_.cap - 1, S.cnts.p);
    BPE_HIP(hipGetLastError());
    BPE_HIP(hipMemcpyAsync(h, S.cnts.p, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    BPE_REQUIRE(!(h[1] & 1u), BPE_E_NOMEM, "accumulator insert hit the probe limit");
    n_words_ += n_new;
    pool_used_ += new_bytes;
}

// the occupied slots of a table over `text` (less the specials) into the scratch record arrays;
// returns how many
size_t WordAccumulator::list_table(const unsigned long long* kv, const unsigned long long* pos, size_t cap,
                                   const uint8_t* text, const std::vector<std::string>& specials) const {
    Scratch& S = *sc_;
    if (!cap) return 0;
    BPE_HIP(hipMemsetAsync(S.n_occ.p, 0, 8, s_));
    BPE_HIP(hipMemsetAsync(S.cnts.p, 0, 8, s_));
    hipLaunchKernelGGL(k_occupied, dim3(grid_for(cap, 256)), dim3(256), 0, s_, kv, cap, S.n_occ.p);
    BPE_HIP(hipGetLastError());
    unsigned long long occ = 0;
    BPE_HIP(hipMemcpyAsync(&occ, S.n_occ.p, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    if (!occ) return 0;
    BPE_REQUIRE(occ < (1ULL << 32), BPE_E_LIMIT, "more than 2^32 words in one table");
    S.w_off.reserve(occ);
    S.w_cnt.reserve(occ);
    S.w_len.reserve(occ);
    std::string spb;
    std::vector<uint32_t> spo, spl;
    for (const auto& s : specials) {
        spo.push_back((uint32_t)spb.size());
        spl.push_back((uint32_t)s.size());
        spb += s;
    }
    S.sp_bytes.reserve(std::max<size_t>(spb.size(), 1));
    S.sp_off.reserve(std::max<size_t>(spo.size(), 1));
    S.sp_len.reserve(std::max<size_t>(spl.size(), 1));
    if (!spb.empty()) BPE_HIP(hipMemcpyAsync(S.sp_bytes.p, spb.data(), spb.size(), hipMemcpyHostToDevice, s_));
    if (!spo.empty()) {
        BPE_HIP(hipMemcpyAsync(S.sp_off.p, spo.data(), spo.size() * 4, hipMemcpyHostToDevice, s_));
        BPE_HIP(hipMemcpyAsync(S.sp_len.p, spl.data(), spl.size() * 4, hipMemcpyHostToDevice, s_));
    }
    hipLaunchKernelGGL(k_list_table, dim3(grid_for(cap, 256)), dim3(256), 0, s_, kv, pos, cap, text, S.sp_bytes.p,
                       S.sp_off.p, S.sp_len.p, (int)specials.size(), S.w_off.p, S.w_len.p, S.w_cnt.p, S.cnts.p,
                       (unsigned)occ);
    BPE_HIP(hipGetLastError());
    unsigned n = 0;
    BPE_HIP(hipMemcpyAsync(&n, S.cnts.p, 4, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));   // (also: the host vectors above are no longer read)
    return n;
}

size_t WordAccumulator::fold(const uint8_t* text, const WordCounts& wc, uint64_t weight) {
    DeviceScope ds(dev_);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = list_table(wc.kv.p, wc.pos.p, wc.cap, text, {});
    fold_list(text, sc_->w_off.p, sc_->w_len.p, sc_->w_cnt.p, n);
    wc_.n_pretokens += wc.n_pretokens;
    weight_ = sat_add(weight_, weight);
    shard_words_ = std::max(shard_words_, n);
    st_.t_fold_ms += ms_from(t0);
    return n;
}

void WordAccumulator::absorb(const WordAccumulator& o) {
    BPE_REQUIRE(&o != this, BPE_E_ARG, "a counter cannot absorb itself");
    BPE_REQUIRE(o.dev_ == dev_, BPE_E_ARG, "the counters live on different devices");
    DeviceScope ds(dev_);
    const auto t0 = std::chrono::steady_clock::now();
    BPE_REQUIRE(sat_add(weight_, o.weight_) < kWeightLimit, BPE_E_LIMIT, "summed counts pass the pair counters' range");
    BPE_HIP(hipStreamSynchronize(o.s_));
    const size_t n = list_table(o.wc_.kv.p, o.wc_.pos.p, o.wc_.cap, o.pool_.p, {});
    fold_list(o.pool_.p, sc_->w_off.p, sc_->w_len.p, sc_->w_cnt.p, n);
    wc_.n_pretokens += o.wc_.n_pretokens;
    weight_ = sat_add(weight_, o.weight_);
    shard_words_ = std::max(shard_words_, o.shard_words_);
    st_.n_inputs += o.st_.n_inputs;
    st_.n_bytes += o.st_.n_bytes;
    st_.n_windows += o.st_.n_windows;
    st_.max_window_bytes = std::max(st_.max_window_bytes, o.st_.max_window_bytes);
    st_.t_load_ms += o.st_.t_load_ms;
    st_.t_count_ms += o.st_.t_count_ms;
    st_.t_fold_ms += o.st_.t_fold_ms + ms_from(t0);
}

// Host records: parsed and checked whole before anything is added, equal words merged (the fold
// needs distinct words), then one packed segment  u64 off[n] | u64 cnt[n] | u32 len[n] | bytes
// goes up in one copy and is folded like a shard's words.
void WordAccumulator::add_records(const uint8_t* blob, size_t n) {
    DeviceScope ds(dev_);
    struct Rec { size_t at; uint32_t len; uint64_t cnt; };
    std::vector<Rec> recs;
    std::unordered_map<std::string_view, size_t> seen;
    uint64_t weight = 0, pretok = 0;
    size_t n_bytes = 0;
    for (size_t off = 0; off < n;) {
        BPE_REQUIRE(n - off >= 4, BPE_E_ARG, "word records: truncated length");
        uint32_t len;
        std::memcpy(&len, blob + off, 4);
        BPE_REQUIRE(n - off - 4 >= (size_t)len && n - off - 4 - len >= 8, BPE_E_ARG, "word records: truncated record");
        BPE_REQUIRE(len < kMaxPretok, BPE_E_LIMIT, "a word of 8 MiB or more");
        uint64_t c;
        std::memcpy(&c, blob + off + 4 + len, 8);
        const size_t at = off + 4;
        off += 12 + (size_t)len;
        if (len < 2 || c == 0) continue;
        uint64_t w;
        if (__builtin_mul_overflow(c, (uint64_t)len, &w)) w = ~0ULL;
        weight = sat_add(weight, w);
        pretok = sat_add(pretok, c);
        const std::string_view key(reinterpret_cast<const char*>(blob + at), len);
        const auto it = seen.find(key);
        if (it != seen.end()) {
            recs[it->second].cnt += c;   // (cannot wrap: the weight check below bounds the sum)
            continue;
        }
        seen.emplace(key, recs.size());
        recs.push_back(Rec{at, len, c});
        n_bytes += len;
    }
    BPE_REQUIRE(sat_add(weight_, weight) < kWeightLimit, BPE_E_LIMIT, "summed counts pass the pair counters' range");
    const size_t m = recs.size();
    st_.n_inputs += 1;
    if (!m) return;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t len_at = 16 * m, bytes_at = (len_at + 4 * m + 7) / 8 * 8;
    std::vector<uint8_t> seg(bytes_at + n_bytes);
    unsigned long long* h_off = reinterpret_cast<unsigned long long*>(seg.data());
    unsigned long long* h_cnt = h_off + m;
    uint32_t* h_len = reinterpret_cast<uint32_t*>(seg.data() + len_at);
    size_t b = 0;
    for (size_t i = 0; i < m; ++i) {
        h_off[i] = b;
        h_cnt[i] = recs[i].cnt;
        h_len[i] = recs[i].len;
        std::memcpy(seg.data() + bytes_at + b, blob + recs[i].at, recs[i].len);
        b += recs[i].len;
    }
    Scratch& S = *sc_;
    S.seg.reserve(seg.size() + kPoolPad);
    BPE_HIP(hipMemcpyAsync(S.seg.p, seg.data(), seg.size(), hipMemcpyHostToDevice, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    fold_list(S.seg.p + bytes_at, reinterpret_cast<const unsigned long long*>(S.seg.p),
              reinterpret_cast<const uint32_t*>(S.seg.p + len_at),
              reinterpret_cast<const unsigned long long*>(S.seg.p) + m, m);
    wc_.n_pretokens += pretok;
    weight_ = sat_add(weight_, weight);
    st_.t_fold_ms += ms_from(t0);
}

void WordAccumulator::export_words(const std::vector<std::string>& specials, uint8_t** blob, size_t* blob_n) const {
    DeviceScope ds(dev_);
    Scratch& S = *sc_;
    const unsigned n = (unsigned)list_table(wc_.kv.p, wc_.pos.p, wc_.cap, pool_.p, specials);
    size_t total = 0;
    if (n) {
        S.len64.reserve(n);
        S.b_off.reserve(n);
        hipLaunchKernelGGL(k_new_lens, dim3(ceil_div(n, 256)), dim3(256), 0, s_, S.w_len.p, (const unsigned*)nullptr, n,
                           S.len64.p, 12ULL);
        exclusive_sum(S.len64.p, S.b_off.p, n, s_, &S.tmp);
        unsigned long long last[2];
        BPE_HIP(hipMemcpyAsync(&last[0], S.b_off.p + n - 1, 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(&last[1], S.len64.p + n - 1, 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        total = (size_t)(last[0] + last[1]);
    }
    uint8_t* out = static_cast<uint8_t*>(std::malloc(std::max<size_t>(total, 1)));
    BPE_REQUIRE(out, BPE_E_NOMEM, "host allocation failed");
    try {
        if (n) {
            S.seg.reserve(total);
            hipLaunchKernelGGL(k_export_write, dim3(ceil_div(n, 256)), dim3(256), 0, s_, pool_.p, S.w_off.p, S.w_len.p,
                               S.w_cnt.p, S.b_off.p, n, S.seg.p);
            BPE_HIP(hipGetLastError());
            BPE_HIP(hipMemcpyAsync(out, S.seg.p, total, hipMemcpyDeviceToHost, s_));
            BPE_HIP(hipStreamSynchronize(s_));
        }
    } catch (...) {
        std::free(out);
        throw;
    }
    *blob = out;
    *blob_n = total;
}

void WordAccumulator::train(int vocab_size, const std::vector<std::string>& specials, TrainOutput& out) const {
    DeviceScope ds(dev_);
    const auto t0 = std::chrono::steady_clock::now();
    BPE_REQUIRE(weight_ < kWeightLimit, BPE_E_LIMIT, "summed counts pass the pair counters' range");
    out = TrainOutput{};
    out.stats.n_bytes = (int64_t)st_.n_bytes;
    out.stats.n_pretokens = (int64_t)wc_.n_pretokens;
    out.stats.t_load_ms = st_.t_load_ms;
    out.stats.t_count_ms = st_.t_count_ms;
    out.stats.n_gpus = 1;
    train_words(pool_.p, wc_, vocab_size, specials, s_, out);
    out.stats.t_total_ms = ms_from(t0);
}

}  // namespace bpe
