// Merge loop, setup and maintenance kernels: word-table build, compaction, the posting index
// build and the rebuild of the candidate list C.
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include "train_apply.h"

namespace bpe {

namespace {

// ------------------------------------------------------------------ word table build
// Occupied count-table slots -> (offset, len, count) words.  Each workgroup takes
// kCollectPer * 256 slots and reserves its words' positions with ONE global atomic (one per
// wave, 262 K same-address atomics at a 16 M-slot table, serialised into ~6 ms).
constexpr unsigned kCollectThreads = 256;
constexpr unsigned kCollectPer = 8;
__global__ void __launch_bounds__(kCollectThreads) k_collect_words(
    const unsigned long long* __restrict__ kv, const unsigned long long* __restrict__ pos, size_t cap,
    const uint8_t* __restrict__ text, const uint8_t* __restrict__ sp_bytes, const uint32_t* __restrict__ sp_off,
    const uint32_t* __restrict__ sp_len, int n_sp, unsigned long long* __restrict__ w_off,
    uint32_t* __restrict__ w_len, unsigned long long* __restrict__ w_cnt, unsigned* __restrict__ n_words,
    unsigned* __restrict__ max_len) {
    __shared__ unsigned s_n, s_base, s_ml;
    if (threadIdx.x == 0) { s_n = 0; s_ml = 0; }
    const size_t s0 = (size_t)blockIdx.x * kCollectThreads * kCollectPer + threadIdx.x;
    unsigned long long key[kCollectPer];
#pragma unroll
    for (unsigned u = 0; u < kCollectPer; ++u) {   // coalesced: slot s0 + u * 256
        const size_t s = s0 + (size_t)u * kCollectThreads;
        key[u] = s < cap ? kv[2 * s] : 0ULL;
    }
    // {key, count} entries (text.hip): the key's top bit marks a word stored inline (length in
    // bits 56..62, an occurrence in pos[]), else key = len << 40 | offset + 1
    unsigned long long off[kCollectPer];
    unsigned len[kCollectPer];
    unsigned mine = 0, ml = 0, keepm = 0;
#pragma unroll
    for (unsigned u = 0; u < kCollectPer; ++u) {
        const size_t s = s0 + (size_t)u * kCollectThreads;
        const unsigned long long k = key[u];
        bool keep = k != 0;
        const bool inl = (k >> 63) != 0;
        len[u] = inl ? (unsigned)((k >> 56) & 0x7f) : (unsigned)(k >> 40);
        off[u] = inl ? (keep ? pos[s] : 0ULL) : (k & ((1ULL << 40) - 1)) - 1;
        for (int i = 0; keep && i < n_sp; ++i) {  // train.py:25 skips matches equal to a special
            if (sp_len[i] != len[u]) continue;
            bool eq = true;
            for (unsigned j = 0; j < len[u] && eq; ++j) eq = text[off[u] + j] == sp_bytes[sp_off[i] + j];
            if (eq) keep = false;
        }
        keepm |= (unsigned)keep << u;
        mine += keep;
        ml = keep && len[u] > ml ? len[u] : ml;
    }
    __syncthreads();   // s_n, s_ml initialised
    const unsigned at = mine ? atomicAdd(&s_n, mine) : 0u;   // LDS: this thread's first position
    ml = wave_max(ml);
    if ((threadIdx.x & 63) == 0 && ml) atomicMax(&s_ml, ml);
    __syncthreads();
    if (threadIdx.x == 0) {
        s_base = s_n ? atomicAdd(n_words, s_n) : 0u;
        if (s_ml) atomicMax(max_len, s_ml);
    }
    __syncthreads();
    unsigned idx = s_base + at;
#pragma unroll
    for (unsigned u = 0; u < kCollectPer; ++u) {
        if (!((keepm >> u) & 1u)) continue;
        const size_t s = s0 + (size_t)u * kCollectThreads;
        w_off[idx] = off[u]; w_len[idx] = len[u]; w_cnt[idx] = kv[2 * s + 1];
        ++idx;
    }
}

__global__ void k_len_u64(const uint32_t* __restrict__ w_len, unsigned n, unsigned long long* __restrict__ o) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = w_len[i];
}

// words -> a CSR of byte ids (the "long" side table)
template <class TokT>
__global__ void k_fill_words(const uint8_t* __restrict__ text, const unsigned long long* __restrict__ w_off,
                             const uint32_t* __restrict__ w_len, const unsigned long long* __restrict__ beg,
                             unsigned n, TokT* __restrict__ tok) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const unsigned long long bg = beg[w];
    const uint32_t len = w_len[w];
    const uint8_t* src = text + w_off[w];
    for (uint32_t i = 0; i < len; ++i) tok[bg + i] = (TokT)src[i];
}

// the initial pair histogram into kHistReplicas copies, so the hottest pairs do not
// serialize on one address
__global__ void k_hist_words(const unsigned long long* __restrict__ w_off, const uint32_t* __restrict__ w_len,
                             const unsigned long long* __restrict__ w_cnt, const uint8_t* __restrict__ text,
                             unsigned n, unsigned long long* __restrict__ hist) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint8_t* src = text + w_off[w];
    const uint32_t len = w_len[w];
    const unsigned long long c = w_cnt[w];
    unsigned long long* h = hist + (size_t)(blockIdx.x % kHistReplicas) * 65536;
    unsigned prev = src[0];
    for (uint32_t i = 1; i < len; ++i) {   // train.py:45-46
        const unsigned cur = src[i];
        atomicAdd(&h[prev * 256 + cur], c);
        prev = cur;
    }
}

__global__ void k_hist_reduce(unsigned long long* __restrict__ hist) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 65536) return;
    unsigned long long s = 0;
    for (int r = 0; r < kHistReplicas; ++r) s += hist[(size_t)r * 65536 + i];
    hist[i] = s;
}

__global__ void k_init_pairs(const unsigned long long* __restrict__ hist, PairsDev P,
                             RoundState* st) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 65536) return;
    const long long c = (long long)hist[i];
    if (c <= 0) return;
    bool ins;
    const size_t s = pair_slot(P, pair_key(i >> 8, i & 255u), st, &ins);
    if (s == ~(size_t)0) return;
    P.cnt[s] = c;
    P.flag[s] = kPresent;
}

__global__ void k_init_tokens(ToksDev K) {
    const unsigned i = threadIdx.x;  // 256 threads
    K.pool[i] = (uint8_t)i;
    K.off[i] = i;
    K.len[i] = 1;
    K.hash[i] = i;
    K.pw[i] = kPolyP;
    K.key8[i] = (unsigned long long)i << 56;
    __syncthreads();
    if (i == 0) {
        for (unsigned t = 0; t < 256; ++t) {
            unsigned s = (unsigned)mix64(t) & K.map_mask;   // a byte token's hash is its byte
            while (K.map[s] != 0) s = (s + 1) & K.map_mask;
            K.map[s] = map_entry(t, t);
        }
    }
}

// ------------------------------------------------------------------ compaction
// flat word index -> (class, index); class kNumCls = long table
template <class TokT>
__device__ __forceinline__ void word_at(const WordsDev<TokT>& W, unsigned g, int* c, unsigned* i) {
    unsigned acc = 0;
    for (int k = 0; k < kNumCls; ++k) {
        if (g < acc + W.c[k].n) { *c = k; *i = g - acc; return; }
        acc += W.c[k].n;
    }
    *c = kNumCls;
    *i = g - acc;
}

template <class TokT>
__device__ __forceinline__ uint32_t word_len(const WordsDev<TokT>& W, int c, unsigned i) {
    return c < kNumCls ? (uint32_t)W.c[c].slot[(size_t)i * slot_w(c)] : W.llen[i];
}

struct MoveCounts {
    unsigned n[kNumCls + 1];
    unsigned fill[kNumCls + 1];
    unsigned long long long_tokens, long_fill;
};

// Compaction in three launches, with no same-address atomics on the hot path: every workgroup
// owns a contiguous range of words; k_move_count writes its per-class counts, k_move_scan turns
// them into per-workgroup bases (one workgroup), k_move places each word at base + running
// offset + rank in its chunk.  Words keep their relative order within a class.
constexpr unsigned kMoveBlocks = 1024;
constexpr int kMoveK = kNumCls + 1;   // destination classes: the slot classes and "long"

__device__ __forceinline__ unsigned move_per_block(unsigned total) { return (total + kMoveBlocks - 1) / kMoveBlocks; }

template <class TokT>
__device__ __forceinline__ int move_class(const WordsDev<TokT>& W, unsigned g, unsigned total, int* c, unsigned* i,
                                          uint32_t* len) {
    int d = -1;
    *len = 0;
    if (g < total) {
        word_at(W, g, c, i);
        *len = word_len(W, *c, *i);
        if (*len >= 2) d = class_for(*len);
    }
    return d;
}

template <class TokT>
__global__ void __launch_bounds__(256) k_move_count(WordsDev<TokT> W, unsigned total, unsigned* __restrict__ blk_cnt,
                                                    MoveCounts* mc) {
    __shared__ unsigned s_c[4][kMoveK];
    const unsigned per = move_per_block(total);
    const unsigned beg = blockIdx.x * per, end = min(total, beg + per);
    unsigned cnt[kMoveK] = {};
    unsigned long long lt = 0;
    for (unsigned g = beg + threadIdx.x; g < end; g += blockDim.x) {
        int c;
        unsigned i;
        uint32_t len;
        const int d = move_class(W, g, total, &c, &i, &len);
#pragma unroll
        for (int k = 0; k < kMoveK; ++k) cnt[k] += d == k;
        if (d == kNumCls) lt += len;
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kMoveK; ++k) {
        const unsigned v = (unsigned)wave_sum((unsigned long long)cnt[k]);
        if ((threadIdx.x & 63) == 0) s_c[wv][k] = v;
    }
    lt = wave_sum(lt);
    if ((threadIdx.x & 63) == 0 && lt) atomicAdd(&mc->long_tokens, lt);
    __syncthreads();
    if (threadIdx.x < kMoveK)
        blk_cnt[blockIdx.x * kMoveK + threadIdx.x] =
            s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x];
}

// one workgroup of kMoveBlocks threads: exclusive scan of every class's per-block counts
__global__ void __launch_bounds__(kMoveBlocks) k_move_scan(unsigned* __restrict__ blk_cnt, MoveCounts* mc) {
    __shared__ unsigned s_w[kMoveBlocks / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int k = 0; k < kMoveK; ++k) {
        const unsigned v = blk_cnt[t * kMoveK + k];
        unsigned x = v;   // inclusive scan in the wave
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        unsigned base = 0;
        for (int w = 0; w < wv; ++w) base += s_w[w];
        blk_cnt[t * kMoveK + k] = base + x - v;   // exclusive
        if (t == kMoveBlocks - 1) mc->n[k] = base + x;
        __syncthreads();
    }
}

template <class TokT>
__global__ void __launch_bounds__(256) k_move(WordsDev<TokT> W, unsigned total, WordsDev<TokT> D,
                                              const unsigned* __restrict__ blk_off, MoveCounts* mc) {
    __shared__ unsigned s_run[kMoveK];        // words of each class placed by earlier chunks
    __shared__ unsigned s_wc[4][kMoveK];      // this chunk: per-wave counts
    const unsigned per = move_per_block(total);
    const unsigned beg = blockIdx.x * per, end = min(total, beg + per);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < kMoveK) s_run[threadIdx.x] = blk_off[blockIdx.x * kMoveK + threadIdx.x];
    for (unsigned g0 = beg; g0 < end; g0 += blockDim.x) {
        const unsigned g = g0 + threadIdx.x;
        int c = 0;
        unsigned i = 0;
        uint32_t len = 0;
        const int d = g < end ? move_class(W, g, total, &c, &i, &len) : -1;
        unsigned rank = 0;
#pragma unroll
        for (int k = 0; k < kMoveK; ++k) {
            const unsigned long long m = __ballot(d == k);
            if (d == k) rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (lane == 0) s_wc[wv][k] = (unsigned)__popcll(m);
        }
        __syncthreads();   // s_run from the previous chunk, s_wc of this one
        unsigned j = ~0u;
        if (d >= 0) {
            unsigned below = 0;
            for (int w = 0; w < wv; ++w) below += s_wc[w][d];
            j = s_run[d] + below + rank;
        }
        __syncthreads();
        if (threadIdx.x < kMoveK)
            s_run[threadIdx.x] += s_wc[0][threadIdx.x] + s_wc[1][threadIdx.x] + s_wc[2][threadIdx.x] + s_wc[3][threadIdx.x];
        if (d < 0) continue;
        const TokT* src = c < kNumCls ? W.c[c].slot + (size_t)i * slot_w(c) + 1 : W.ltok + W.lbeg[i];
        const unsigned long long cnt = c < kNumCls ? W.c[c].cnt[i] : W.lcnt[i];
        if (d < kNumCls) {
            TokT* dst = D.c[d].slot + (size_t)j * slot_w(d);
            dst[0] = (TokT)len;
            for (uint32_t k = 0; k < len; ++k) dst[1 + k] = src[k];
            for (int k = (int)len + 1; k < slot_w(d); ++k) dst[k] = sentinel<TokT>();
            D.c[d].cnt[j] = cnt;
        } else {
            const unsigned long long bg = atomicAdd(&mc->long_fill, (unsigned long long)len);
            for (uint32_t k = 0; k < len; ++k) D.ltok[bg + k] = src[k];
            D.lbeg[j] = bg;
            D.llen[j] = len;
            D.lcnt[j] = cnt;
        }
    }
}

// ------------------------------------------------------------------ posting index build
template <class TokT>
__device__ __forceinline__ const TokT* slot_of(const WordsDev<TokT>& W, unsigned f, uint32_t* len) {
    int c = 0;
    while (c + 1 < kNumCls && f >= W.off[c + 1]) ++c;
    const TokT* s = W.c[c].slot + (size_t)(f - W.off[c]) * slot_w(c);
    *len = s[0];
    return s + 1;
}

// Two passes per slot class (count each word's distinct tokens, then emit them at the scanned
// positions), the slot in registers (one 16-byte load per 16 bytes of slot, every index a
// compile-time constant): the first occurrence of each token of a word is a register compare, not
// a dependent load per pair
template <class TokT, int C, bool kEmit>
__global__ void __launch_bounds__(256) k_index_cls(WordsDev<TokT> W, const uint32_t* __restrict__ pos,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ vals) {
    constexpr int Wd = slot_w(C);
    constexpr int V = Wd * (int)sizeof(TokT) / 16;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W.c[C].n) return;
    const unsigned f = W.off[C] + i;
    uint4 r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = reinterpret_cast<const uint4*>(W.c[C].slot + (size_t)i * Wd)[v];
    TokT e[Wd];
    __builtin_memcpy(e, r, sizeof(e));
    const uint32_t len = e[0];
    uint32_t o = kEmit ? pos[f] : 0u, d = 0;
    if (len >= 2) {
#pragma unroll
        for (int k = 1; k < Wd; ++k) {   // no early exit: a constant trip count keeps e[] in registers
            bool first = (uint32_t)k <= len;
#pragma unroll
            for (int q = 1; q < k; ++q) first &= e[q] != e[k];
            if (first) {
                if (kEmit) { keys[o] = e[k]; vals[o] = f; ++o; }
                else ++d;
            }
        }
    }
    if (!kEmit) cnt[f] = d;
}

template <class TokT, bool kEmit>
void index_pass(const WordsDev<TokT>& W, const uint32_t* pos, uint32_t* cnt, uint32_t* keys, uint32_t* vals,
                hipStream_t s) {
    if (W.c[0].n) hipLaunchKernelGGL((k_index_cls<TokT, 0, kEmit>), dim3(ceil_div(W.c[0].n, 256u)), dim3(256), 0, s, W, pos, cnt, keys, vals);
    if (W.c[1].n) hipLaunchKernelGGL((k_index_cls<TokT, 1, kEmit>), dim3(ceil_div(W.c[1].n, 256u)), dim3(256), 0, s, W, pos, cnt, keys, vals);
    if (W.c[2].n) hipLaunchKernelGGL((k_index_cls<TokT, 2, kEmit>), dim3(ceil_div(W.c[2].n, 256u)), dim3(256), 0, s, W, pos, cnt, keys, vals);
    if (W.c[3].n) hipLaunchKernelGGL((k_index_cls<TokT, 3, kEmit>), dim3(ceil_div(W.c[3].n, 256u)), dim3(256), 0, s, W, pos, cnt, keys, vals);
}

__global__ void k_index_bounds(const uint32_t* __restrict__ keys, unsigned long long e,
                               uint32_t* __restrict__ beg, uint32_t* __restrict__ len) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e) return;
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) beg[k] = (uint32_t)i;
    if (i + 1 == e || keys[i + 1] != k) len[k] = (uint32_t)(i + 1);   // end; beg subtracted below
}

__global__ void k_index_lens(const uint32_t* __restrict__ beg, uint32_t* __restrict__ len, unsigned ntok) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntok && len[t]) len[t] -= beg[t];
}


// ------------------------------------------------------------------ rebuild helpers
struct RebuildStats {
    unsigned long long bins[64];
    unsigned long long ghosts;
    unsigned long long sub[1024];
};

__global__ void k_rebuild_hist(PairsDev P, size_t cap, RebuildStats* rs) {
    __shared__ unsigned long long sh[64];
    if (threadIdx.x < 64) sh[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long ghosts = 0;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap;
         s += (size_t)gridDim.x * blockDim.x) {
        if (!(P.flag[s] & kPresent)) continue;
        const long long c = P.cnt[s];
        if (c <= 0) { ghosts += (c == 0); continue; }
        atomicAdd(&sh[63 - __clzll((unsigned long long)c)], 1ULL);
    }
    ghosts = wave_sum(ghosts);
    if ((threadIdx.x & 63) == 0 && ghosts) atomicAdd(&rs->ghosts, ghosts);
    __syncthreads();
    if (threadIdx.x < 64 && sh[threadIdx.x]) atomicAdd(&rs->bins[threadIdx.x], sh[threadIdx.x]);
}

__global__ void k_rebuild_sub(PairsDev P, size_t cap, long long lo, long long hi, long long width,
                              RebuildStats* rs) {
    __shared__ unsigned sh[1024];
    for (int k = threadIdx.x; k < 1024; k += blockDim.x) sh[k] = 0;
    __syncthreads();
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap;
         s += (size_t)gridDim.x * blockDim.x) {
        if (!(P.flag[s] & kPresent)) continue;
        const long long c = P.cnt[s];
        if (c < lo || c >= hi) continue;
        atomicAdd(&sh[(c - lo) / width], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 1024; k += blockDim.x)
        if (sh[k]) atomicAdd(&rs->sub[k], (unsigned long long)sh[k]);
}

__global__ void k_build_C(PairsDev P, size_t cap, long long T, RoundState* st) {
    for (size_t s0 = (size_t)blockIdx.x * blockDim.x; s0 < cap; s0 += (size_t)gridDim.x * blockDim.x) {
        const size_t s = s0 + threadIdx.x;
        const unsigned f = s < cap ? P.flag[s] : 0u;
        const bool in = (f & kPresent) && P.cnt[s] >= T;
        const unsigned idx = wave_append(in, &st->nC);
        if (in) {
            const unsigned long long key = P.key[s] - 1ULL;
            if (idx < st->capC) P.C[idx] = make_uint4((unsigned)s, (unsigned)(key >> 32), (unsigned)key, 0u);
            else atomicOr(&st->err, ERR_C_FULL);
            if (!(f & kInC)) P.flag[s] = f | kInC;
        } else if (f & kInC) {
            P.flag[s] = f & ~kInC;
        }
    }
}

__global__ void k_collect_present(PairsDev P, size_t cap, unsigned long long* out,
                                  unsigned* n_out) {
    for (size_t s0 = (size_t)blockIdx.x * blockDim.x; s0 < cap; s0 += (size_t)gridDim.x * blockDim.x) {
        const size_t s = s0 + threadIdx.x;
        const bool in = s < cap && (P.flag[s] & kPresent);
        const unsigned idx = wave_append(in, n_out);
        if (in) out[idx] = P.key[s] - 1ULL;
    }
}

__global__ void k_rehash(const unsigned long long* __restrict__ okey, const long long* __restrict__ ocnt,
                         const unsigned* __restrict__ oflag, size_t ocap, PairsDev P, RoundState* st) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ocap) return;
    const unsigned long long k = okey[i];
    if (!k) return;
    bool ins;
    const size_t s = pair_slot(P, k, st, &ins);
    if (s == ~(size_t)0) return;
    P.cnt[s] = ocnt[i];
    P.flag[s] = oflag[i] & kPresent;
}

}  // namespace

}  // namespace bpe
