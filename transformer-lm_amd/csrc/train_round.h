// Merge loop, per-round kernels: word rewrites, the slot-class scan, k_merge,
// k_apply_argmax and k_argmax (BPE355_BATCH=0 and the sharded per-round exchange run them).
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include "train_state.h"

namespace bpe {

namespace {

// ------------------------------------------------------------------ word rewrite
// The reference's in-place merge of one word (train.py:196-224): t[0..len) -> t[0..j).
// Per occurrence: the left neighbour is already rewritten (t[j-1]); the right one is the
// original t[r+2].  With `pad`, the freed tail is refilled with the sentinel.
// Per-occurrence deltas are keyed by the neighbour token: cell 2x = L[x] for (x,a)-=c and
// (x,new)+=c, cell 2x+1 = R[x] for (b,x)-=c and (new,x)+=c.  Cells of ids below kLdsLR (the
// bytes and the first merges: neighbours hot enough to serialize a global atomic) are summed
// in LDS per workgroup and flushed once; the others go out directly.
constexpr unsigned kLdsLR = 512;

// (Applying the four pair updates of a cell inside the merge kernel instead was measured
// slower: one hit's updates form a serial chain on one thread; see DESIGN.md.)
typedef __attribute__((address_space(3))) unsigned long long LdsU64;   // an LDS cell
struct DeltaSink {
    unsigned long long* LR;     // global delta cells (all-reduced when sharded) for k_apply
    LdsU64* lds;
    __device__ __forceinline__ void add(unsigned cell, unsigned long long c) const {
        if (cell < 2 * kLdsLR) __hip_atomic_fetch_add(&lds[cell], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else atomicAdd(&LR[cell], c);
    }
};

template <class TokT, class Sink>
__device__ __forceinline__ uint32_t rewrite_word(TokT* __restrict__ t, uint32_t len, TokT a, TokT b,
                                                 TokT nw, unsigned long long c, const Sink& D, bool pad) {
    uint32_t j = 0, r = 0;
    while (r < len) {
        const TokT x = t[r];
        if (x == a && r + 1 < len && t[r + 1] == b) {
            if (j > 0) D.add(2u * (unsigned)t[j - 1], c);           // (x,a)-=c, (x,new)+=c
            if (r + 2 < len) D.add(2u * (unsigned)t[r + 2] + 1, c);  // (b,y)-=c, (new,y)+=c
            t[j++] = nw;
            r += 2;
        } else {
            t[j++] = x;
            ++r;
        }
    }
    if (pad)
        for (uint32_t k = j; k < len; ++k) t[k] = sentinel<TokT>();
    return j;
}

// rewrite_word for a slot word already in registers (e: the slot, e[0] = length, sentinel-padded):
// the matches are found on the registers (every index a compile-time constant), so the only
// memory traffic is the stores of the shifted tail, not a load per token
template <class TokT, int W, class Sink>
__device__ __forceinline__ uint32_t rewrite_slot(const TokT (&e)[W], TokT* __restrict__ s, TokT a, TokT b,
                                                 TokT nw, unsigned long long c, const Sink& D) {
    const TokT sent = sentinel<TokT>();
    uint32_t j = 0;      // output tokens so far
    TokT prev = sent;    // the last output token
    bool skip = false;   // this position is the b of the previous match
#pragma unroll
    for (int q = 1; q < W; ++q) {
        const TokT x = e[q];
        if (x == sent) break;
        if (skip) { skip = false; continue; }
        if (q + 1 < W && x == a && e[q + 1 < W ? q + 1 : q] == b) {
            if (j > 0) D.add(2u * (unsigned)prev, c);                      // (x,a)-=c, (x,new)+=c
            if (q + 2 < W && e[q + 2 < W ? q + 2 : q] != sent)
                D.add(2u * (unsigned)e[q + 2 < W ? q + 2 : q] + 1, c);     // (b,y)-=c, (new,y)+=c
            s[1 + j] = nw;
            prev = nw;
            skip = true;
        } else {
            if (j != (uint32_t)(q - 1)) s[1 + j] = x;
            prev = x;
        }
        ++j;
    }
    for (uint32_t p = j; p < (uint32_t)e[0]; ++p) s[1 + p] = sent;
    s[0] = (TokT)j;
    return j;
}

// Several members' rewrites of one slot word in registers, then one compacting store (batched
// trips).  rewrite_slot per member needed the word re-read from memory between members: a
// dependent load per extra member on the thread's chain.  Here member j's matches replace
// e[q] by new_j and leave a hole at q + 1 (a bit of `hole`, its value the sentinel), so every
// index stays a compile-time constant.  A hole only ever follows a new token, which is no
// member's a or b, so no match spans a hole and no hole starts a match; the left neighbour of a
// match is e[q - 1], or e[q - 2] behind a hole; the right one is e[q + 2] (e[q + 1] is b, an
// old token, so q + 2 is never a hole).  Matches of one member cannot overlap (a != b for
// k > 1), and the ascending pass sees the already-rewritten left and the original right, as
// rewrite_word (the reference's loop, train.py:196-224) does.  Returns the new length.
template <class TokT, int W, class PA, class SinkOf>
__device__ __forceinline__ uint32_t rewrite_slot_members(TokT (&e)[W], TokT* __restrict__ s, unsigned hits,
                                                         PA ta, PA tb, PA tn,
                                                         unsigned long long c, const SinkOf& sink_of) {
    static_assert(W <= 64, "one hole bit per position");
    const TokT sent = sentinel<TokT>();
    const uint32_t len0 = (uint32_t)e[0];
    unsigned long long hole = 0, chg = 0;
    while (hits) {
        const int j = __builtin_ctz(hits);
        hits &= hits - 1;
        const TokT a = (TokT)ta[j], b = (TokT)tb[j], nw = (TokT)tn[j];
        const auto D = sink_of(j);
#pragma unroll
        for (int q = 1; q + 1 < W; ++q) {
            if (e[q] == a && e[q + 1] == b) {
                if (q > 1) {
                    // e[q - 1], or e[q - 2] behind a hole (arithmetic, not a select of two array
                    // loads, which would keep e[] out of registers)
                    unsigned left = (unsigned)e[q - 1];
                    if (q > 2) {
                        const unsigned h = 0u - (unsigned)((hole >> (q - 1)) & 1);
                        left ^= (left ^ (unsigned)e[q > 2 ? q - 2 : 1]) & h;
                    }
                    D.add(2u * left, c);                                          // (x,a)-=c, (x,new)+=c
                }
                if (q + 2 < W && e[q + 2 < W ? q + 2 : q] != sent)
                    D.add(2u * (unsigned)e[q + 2 < W ? q + 2 : q] + 1, c);        // (b,y)-=c, (new,y)+=c
                e[q] = nw;
                e[q + 1] = sent;
                hole |= 1ull << (q + 1);
                chg |= 1ull << q;
            }
        }
    }
    uint32_t j = 0;   // output tokens so far
#pragma unroll
    for (int q = 1; q < W; ++q) {   // (no early exit: a data-dependent one un-unrolls the loop)
        if ((uint32_t)q <= len0 && !((hole >> q) & 1)) {
            if (j != (uint32_t)(q - 1) || ((chg >> q) & 1)) s[1 + j] = e[q];
            ++j;
        }
    }
    for (uint32_t p = j; p < len0; ++p) s[1 + p] = sent;
    s[0] = (TokT)j;
    return j;
}

// scan one slot class: U words in flight per thread, one 16-byte load per 16 bytes of slot
template <class TokT, int C, class Sink>
__device__ __forceinline__ void scan_class(const SlotCls<TokT>& S, unsigned bi, TokT a, TokT b,
                                           TokT nw, const Sink& D, unsigned& singles) {
    constexpr int W = slot_w(C);
    constexpr int V = W * (int)sizeof(TokT) / 16;
    constexpr int U = V == 1 ? 4 : (V == 2 ? 2 : 1);
    const unsigned stride = S.nblk * blockDim.x;
    for (unsigned base = bi * blockDim.x + threadIdx.x; base < S.n; base += stride * U) {
        uint4 r[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned i = base + u * stride;
#pragma unroll
            for (int v = 0; v < V; ++v)
                r[u][v] = i < S.n ? reinterpret_cast<const uint4*>(S.slot + (size_t)i * W)[v]
                                  : make_uint4(~0u, ~0u, ~0u, ~0u);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned i = base + u * stride;
            TokT e[W];
            __builtin_memcpy(e, r[u], sizeof(e));
            bool hit = false;
#pragma unroll
            for (int k = 1; k + 1 < W; ++k) hit |= (e[k] == a) & (e[k + 1] == b);
            if (hit) {
                const uint32_t j = rewrite_slot(e, S.slot + (size_t)i * W, a, b, nw, S.cnt[i], D);
                singles += (j < 2);
            }
        }
    }
}

// one word of class C addressed directly (index-list mode)
template <class TokT, int C, class Sink>
__device__ __forceinline__ void merge_one(const SlotCls<TokT>& S, unsigned i, TokT a, TokT b,
                                          TokT nw, const Sink& D, unsigned& singles) {
    constexpr int W = slot_w(C);
    constexpr int V = W * (int)sizeof(TokT) / 16;
    uint4 r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = reinterpret_cast<const uint4*>(S.slot + (size_t)i * W)[v];
    const unsigned long long c = S.cnt[i];   // issued with the slot: no extra dependent load on a hit
    TokT e[W];
    __builtin_memcpy(e, r, sizeof(e));
    bool hit = false;
#pragma unroll
    for (int k = 1; k + 1 < W; ++k) hit |= (e[k] == a) & (e[k + 1] == b);
    if (hit) {
        const uint32_t j = rewrite_slot(e, S.slot + (size_t)i * W, a, b, nw, c, D);
        singles += (j < 2);
    }
}

// ------------------------------------------------------------------ K1: merge
struct BestShared {
    int stop;
    unsigned a, b, nw, slot, isnew;
    long long cnt;
    unsigned long long hash, k8;
    int round, ntok;
    unsigned ln, list_beg, list_len, use_list, cov_beg, cov_len;
};

template <class TokT>
__global__ void __launch_bounds__(256) k_merge(RoundState* __restrict__ st,
                                               const Partial* __restrict__ part, int nparts,
                                               PairsDev P, ToksDev K, WordsDev<TokT> W,
                                               IndexDev X, unsigned long long* __restrict__ LR,
                                               uint32_t* __restrict__ m_a, uint32_t* __restrict__ m_b,
                                               uint32_t* __restrict__ m_new, uint32_t* __restrict__ m_mode,
                                               long long* __restrict__ m_cnt) {
    __shared__ BestShared sb;
    __shared__ unsigned long long l_lr[2 * kLdsLR];
    __shared__ Cand s_part[4];
    const int tid = threadIdx.x;
    for (unsigned k = tid; k < 2 * kLdsLR; k += blockDim.x) l_lr[k] = 0;
    {   // all four waves reduce the argmax partials (a few independent loads per thread)
        Cand pp = cand_none();
        for (int i = tid; i < nparts; i += blockDim.x) {
            const Partial q = part[i];
            const Cand c{q.cnt, q.ka, q.kb, q.slot, q.a, q.b};
            if (cand_better(c, pp, K.pool, K.off, K.len)) pp = c;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const Cand oc = shfl_xor_cand(pp, o);
            if (cand_better(oc, pp, K.pool, K.off, K.len)) pp = oc;
        }
        if ((tid & 63) == 0) s_part[tid >> 6] = pp;
    }
    __syncthreads();
    if (tid < 64) {
        // Every workgroup redundantly decides the round (no extra launch, no grid sync).  The
        // loads are grouped by dependency level so the chain is ~4 memory latencies long:
        // state + partials | token metadata, posting-list ids | map slot, list bounds | (dedupe)
        const int halt = st->halt, round = st->round, ntok = st->ntok;
        const int n_rounds = st->n_rounds;
        const unsigned nC = st->nC, c_limit = st->c_limit;   // only k_apply_argmax appends to C
        const long long T = st->T;
        Cand pp = s_part[0];
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (cand_better(s_part[k], pp, K.pool, K.off, K.len)) pp = s_part[k];
        int stop = HALT_NONE;
        if (halt) stop = -1;
        else if (round >= n_rounds) stop = HALT_DONE;
        else if (nC > c_limit) stop = HALT_REBUILD;   // C bloated: re-threshold
        else if (pp.cnt < T) stop = HALT_REBUILD;     // max(C) < T: re-threshold
        if (tid == 0) {
            sb.stop = stop;
            if (!stop) {
                const unsigned a = pp.a, b = pp.b;
                // level 1: everything keyed by a or b
                const unsigned long long ha = K.hash[a], pb = K.pw[b], hb = K.hash[b];
                const unsigned la = K.len[a], lb = K.len[b];
                const unsigned long long ka = pp.ka, kb = pp.kb;
                const unsigned za = X.len[a], zb = X.len[b];   // kNoAnc (uncovered) sorts last
                const unsigned ba = X.beg[a], bbg = X.beg[b];
                sb.a = a; sb.b = b; sb.slot = pp.slot; sb.cnt = pp.cnt;
                sb.hash = ha * pb + hb;
                sb.ln = la + lb;
                sb.k8 = la >= 8 ? ka : (ka | (kb >> (8 * la)));
                sb.round = round; sb.ntok = ntok;
                // which words can contain (a, b): the smaller covering posting list, or all
                const bool pick_a = za <= zb;
                const unsigned lu = pick_a ? za : zb, bu = pick_a ? ba : bbg;
                sb.use_list = lu != kNoAnc && lu <= X.full_threshold;
                sb.list_beg = sb.use_list ? bu : 0;
                sb.list_len = sb.use_list ? lu : 0;
                sb.cov_beg = bu;
                sb.cov_len = lu;
            }
        }
    }
    __syncthreads();
    if (sb.stop) {
        if (blockIdx.x == 0 && tid == 0 && sb.stop > 0) st->halt = sb.stop;
        return;
    }
    // While thread 0 resolves the new token's id (token dedupe: does bytes(a) + bytes(b) exist
    // already? usually an empty map slot), every thread pulls its first posting-list entry and
    // that word's slot line toward the CU; the barrier below waits for both.
    {
        const unsigned i = blockIdx.x * blockDim.x + tid;
        if (sb.use_list && blockIdx.x < W.lblk0 && i < sb.list_len) {
            const unsigned f = X.list[sb.list_beg + i];
            const TokT* line = f < W.off[1] ? W.c[0].slot + (size_t)f * slot_w(0)
                             : f < W.off[2] ? W.c[1].slot + (size_t)(f - W.off[1]) * slot_w(1)
                             : f < W.off[3] ? W.c[2].slot + (size_t)(f - W.off[2]) * slot_w(2)
                                            : W.c[3].slot + (size_t)(f - W.off[3]) * slot_w(3);
            (void)*reinterpret_cast<const volatile unsigned*>(line);   // kept: volatile
        }
        if (tid == 0) {
            const unsigned a = sb.a, b = sb.b, ln = sb.ln, ntok = (unsigned)sb.ntok;
            const unsigned long long h = sb.hash;
            const unsigned old = map_find(K, h, ln, a, b);
            const unsigned nw = old != ~0u ? old : ntok;
            sb.nw = nw;
            sb.isnew = nw == ntok;
            if (!sb.isnew) sb.cov_len = kNoAnc;   // dedupe: uncovered until the next build
        }
    }
    __syncthreads();
    const unsigned a = sb.a, b = sb.b, nw = sb.nw;

    if (blockIdx.x == 0) {  // record the merge, pop the pair, register a new token
        if (tid == 0) {
            st->nC_base = st->nC;     // C entries k_apply_argmax may scan without racing its appends
            st->cur_round = sb.round;
            st->cur_ntok = sb.ntok + (int)sb.isnew;
            P.cnt[sb.slot] = 0;                       // byte_pair_frequencies.pop(best_pair)
            atomicAnd(&P.flag[sb.slot], ~kPresent);   // (no other update touches this key)
            st->cur_a = a; st->cur_b = b; st->cur_new = nw; st->cur_slot = sb.slot;
            st->cur_cnt = sb.cnt; st->new_is_new = (int)sb.isnew;
            m_a[sb.round] = a; m_b[sb.round] = b; m_new[sb.round] = nw;
            if (m_cnt) m_cnt[sb.round] = sb.cnt;
            m_mode[sb.round] = sb.use_list ? sb.list_len : 0xffffffffu;
            X.beg[nw] = sb.cov_beg;
            X.len[nw] = sb.cov_len;
        }
        if (sb.isnew) {
            const unsigned la = K.len[a], ln = la + K.len[b];
            const unsigned base = st->pool_used;
            if (base + ln <= st->pool_cap) {
                for (unsigned i = tid; i < ln; i += blockDim.x)
                    K.pool[base + i] = concat_byte(K, a, la, b, i);
            }
            __syncthreads();
            if (tid == 0) {
                if (base + ln > st->pool_cap) atomicOr(&st->err, ERR_POOL);
                K.off[nw] = base; K.len[nw] = ln;
                K.hash[nw] = sb.hash; K.pw[nw] = K.pw[a] * K.pw[b]; K.key8[nw] = sb.k8;
                st->pool_used = base + ln;
            }
        }
    }

    // rewrite every word containing (a, b): this block's share of one slot class
    unsigned singles = 0;
    const unsigned bid = blockIdx.x;
    const TokT ta = (TokT)a, tb = (TokT)b, tn = (TokT)nw;
    const DeltaSink D{LR, (LdsU64*)l_lr};
    if (sb.use_list && bid < W.lblk0) {
        // index mode: only the words on the posting list (a gather of their slots)
        const uint32_t* L = X.list + sb.list_beg;
        for (unsigned i = bid * blockDim.x + tid; i < sb.list_len; i += W.lblk0 * blockDim.x) {
            const unsigned f = L[i];
            if (f < W.off[1]) merge_one<TokT, 0>(W.c[0], f, ta, tb, tn, D, singles);
            else if (f < W.off[2]) merge_one<TokT, 1>(W.c[1], f - W.off[1], ta, tb, tn, D, singles);
            else if (f < W.off[3]) merge_one<TokT, 2>(W.c[2], f - W.off[2], ta, tb, tn, D, singles);
            else merge_one<TokT, 3>(W.c[3], f - W.off[3], ta, tb, tn, D, singles);
        }
    } else if (bid < W.c[1].blk0) {
        if (bid < W.c[0].blk0 + W.c[0].nblk)
            scan_class<TokT, 0>(W.c[0], bid - W.c[0].blk0, ta, tb, tn, D, singles);
    } else if (bid < W.c[2].blk0) {
        scan_class<TokT, 1>(W.c[1], bid - W.c[1].blk0, ta, tb, tn, D, singles);
    } else if (bid < W.c[3].blk0) {
        scan_class<TokT, 2>(W.c[2], bid - W.c[2].blk0, ta, tb, tn, D, singles);
    } else if (bid < W.lblk0) {
        scan_class<TokT, 3>(W.c[3], bid - W.c[3].blk0, ta, tb, tn, D, singles);
    } else if (bid < W.lblk0 + W.lnblk) {
        for (unsigned i = (bid - W.lblk0) * blockDim.x + tid; i < W.ln; i += W.lnblk * blockDim.x) {
            const uint32_t len = W.llen[i];
            if (len < 2) continue;
            TokT* t = W.ltok + W.lbeg[i];
            bool hit = false;
            for (uint32_t k = 0; k + 1 < len && !hit; ++k) hit = (t[k] == ta) & (t[k + 1] == tb);
            if (!hit) continue;
            const uint32_t j = rewrite_word(t, len, ta, tb, tn, W.lcnt[i], D, false);
            W.llen[i] = j;
            singles += (j < 2);
        }
    }
    singles = wave_sum(singles);   // words that became one token (rare: no contention)
    if ((tid & 63) == 0 && singles) atomicAdd(&st->n_single, singles);
    __syncthreads();
    for (unsigned k = tid; k < 2 * kLdsLR; k += blockDim.x) {
        const unsigned long long v = l_lr[k];
        if (v) atomicAdd(&LR[k], v);
    }
}

// ------------------------------------------------------------------ K2: apply + argmax
// One launch applies the round's deltas and takes the argmax for the next round.
//  * cell threads (4 per token x, op = g & 3):  0 (x,a) -= L[x]   1 (x,new) += L[x]
//                                               2 (b,x) -= R[x]   3 (new,x) += R[x]
//    Only four keys can receive two of these updates -- (b,a), (b,new), (new,a), (new,new) --
//    and thread 0 applies those; every other key has ONE updater, so counts are updated with
//    plain loads/stores and the updater sees the key's final count: it evaluates the key for
//    the argmax and admits it to C when an increment lifts it to T (identical on every rank).
//  * C threads scan the candidate list C (entries before this round's appends).  An entry is
//    skipped iff this round's cells touch it -- exactly the rule above -- and its updater
//    evaluates it instead; the others' counts do not change during the launch.
// The cells are double-buffered by round parity: this launch reads LR (this round) and clears
// LRold (the previous round's, already applied).  Round state is written only into fields the
// other kernel reads (k_merge -> cur_*, this kernel -> round/ntok), so no grid-wide ordering.
// apply `delta` to the key (p, q) (its only updater this round); present if incremented or
// created (a decrement of a missing key creates it, as the reference's defaultdict does)
__device__ __forceinline__ size_t pair_update(const PairsDev& P, RoundState* st, unsigned p, unsigned q,
                                              long long delta, bool inc, long long* c_out, unsigned* f_out) {
    const unsigned long long key = pair_key(p, q);
    const size_t s0 = mix64(key) & P.mask;
    // the home slot's key, count and flags in one step: at load <= 1/2 the first probe usually
    // decides, so the usual chain is one dependent load
    const unsigned long long k0 = P.key[s0];
    long long c = P.cnt[s0];
    unsigned f = P.flag[s0];
    bool ins = false;
    size_t s = s0;
    if (k0 != key) {
        s = pair_slot(P, key, st, &ins);
        if (s == ~(size_t)0) return s;
        if (ins) {          // a slot this call claimed was empty: count and flags are 0
            c = 0;
            f = 0;
        } else {
            c = P.cnt[s];
            f = P.flag[s];
        }
    }
    c += delta;
    P.cnt[s] = c;
    if ((inc || ins) && !(f & kPresent)) {
        f |= kPresent;
        P.flag[s] = f;
    }
    *c_out = c;
    *f_out = f;
    return s;
}

// pair_update with the home slot's key, count and flags already loaded (k0, c0, f0): the
// caller issues several keys' home-slot loads before finishing any of them
// Inserted keys are counted in *n_ins (the caller adds them to st->pair_used once per workgroup:
// one same-address atomic per insert serialises thousands of them at the end of a trip).
__device__ __forceinline__ size_t pair_update_from(const PairsDev& P, RoundState* st, unsigned p, unsigned q,
                                                   long long delta, bool inc, unsigned long long k0, long long c0,
                                                   unsigned f0, long long* c_out, unsigned* f_out, unsigned& n_ins) {
    const unsigned long long key = pair_key(p, q);
    size_t s = mix64(key) & P.mask;
    long long c = c0;
    unsigned f = f0;
    bool ins = false;
    if (k0 != key) {   // the probe from the home slot on, its first key already known
        unsigned long long k = k0;
        size_t probe = 0;
        for (;;) {
            if (k == key) break;
            if (k == 0) {
                k = atomicCAS(&P.key[s], 0ULL, key);
                if (k == 0) {
                    ++n_ins;
                    ins = true;
                    break;
                }
                if (k == key) break;
            }
            if (++probe > P.mask) {
                atomicOr(&st->err, ERR_PAIRS_FULL);
                return ~(size_t)0;
            }
            s = (s + 1) & P.mask;
            k = P.key[s];
        }
        if (ins) {          // a slot this call claimed was empty: count and flags are 0
            c = 0;
            f = 0;
        } else {
            c = P.cnt[s];
            f = P.flag[s];
        }
    }
    c += delta;
    P.cnt[s] = c;
    if ((inc || ins) && !(f & kPresent)) {
        f |= kPresent;
        P.flag[s] = f;
    }
    *c_out = c;
    *f_out = f;
    return s;
}

constexpr unsigned kApplyThreads = 256;    // large workgroups: fewer argmax partials for k_merge
__global__ void __launch_bounds__(kApplyThreads) k_apply_argmax(RoundState* __restrict__ st, PairsDev P, ToksDev K,
                                                      const unsigned long long* __restrict__ LR,
                                                      unsigned long long* __restrict__ LRold,
                                                      unsigned ntb, unsigned cell_blocks,
                                                      Partial* __restrict__ part) {
    __shared__ Cand sw[kApplyThreads / 64];
    const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool cell_thread = blockIdx.x < cell_blocks;
    const unsigned x = g >> 2, op = g & 3;
    // the cell load needs no state (ntb bounds every id k_merge can have written)
    const long long d = cell_thread && x < ntb ? (long long)LR[2 * (size_t)x + (op >> 1)] : 0;
    if (cell_thread && (op & 1) && x < ntb) LRold[2 * (size_t)x + (op >> 1)] = 0;
    Cand best = cand_none();
    if (!st->halt) {
        const unsigned a = st->cur_a, b = st->cur_b, nw = st->cur_new;
        const long long T = st->T;
        // a key this thread updated: candidate if present and >= T; increments may admit it
        auto consider = [&](size_t s, unsigned p, unsigned q, unsigned long long ka, unsigned long long kb,
                            long long c, unsigned f, bool inc) -> bool {
            if (s == ~(size_t)0 || !(f & kPresent) || c < T) return false;
            const Cand cand{c, ka, kb, (unsigned)s, p, q};
            if (cand_better(cand, best, K.pool, K.off, K.len)) best = cand;
            if (inc && !(f & kInC)) {
                P.flag[s] = f | kInC;
                return true;
            }
            return false;
        };
        bool add = false;
        uint4 add_e = make_uint4(0, 0, 0, 0);
        if (cell_thread) {
            if (d) {
                const bool special = (op <= 1) ? (x == b || x == nw) : (x == a || x == nw);
                const bool popped = (op == 0 && x == a && a == b) || (op == 2 && x == b && a == b);
                if (!special && !popped) {
                    const unsigned p = op == 0 ? x : op == 1 ? x : op == 2 ? b : nw;
                    const unsigned q = op == 0 ? a : op == 1 ? nw : x;
                    const bool inc = op & 1;
                    const unsigned long long ka = K.key8[p], kb = K.key8[q];   // issued with the probe
                    long long c;
                    unsigned f;
                    const size_t s = pair_update(P, st, p, q, inc ? d : -d, inc, &c, &f);
                    if (consider(s, p, q, ka, kb, c, f, inc)) { add = true; add_e = make_uint4((unsigned)s, p, q, 0u); }
                }
            }
            if (g == 0) {   // the four keys two cells can update
                const long long Lb = (long long)LR[2 * (size_t)b], Ln = (long long)LR[2 * (size_t)nw];
                const long long Ra = (long long)LR[2 * (size_t)a + 1], Rn = (long long)LR[2 * (size_t)nw + 1];
                struct Sp { unsigned p, q; long long dec, inc; };
                const Sp sp[4] = {{b, a, a == b ? 0 : Lb + Ra, 0},   // (a,b) itself when a == b: popped
                                  {b, nw, Rn, Lb},
                                  {nw, a, Ln, Ra},
                                  {nw, nw, 0, Ln + Rn}};
                // (the decrements use the same cells as their single-updater twins above)
                for (int k = 0; k < 4; ++k) {
                    const bool touched = (k == 0) ? (a != b && (Lb || Ra))
                                       : (k == 1) ? (Lb || Rn)
                                       : (k == 2) ? (Ln || Ra)
                                                  : (Ln || Rn);
                    if (!touched) continue;
                    long long c;
                    unsigned f;
                    const bool inc = sp[k].inc != 0;
                    const size_t s = pair_update(P, st, sp[k].p, sp[k].q, sp[k].inc - sp[k].dec, inc, &c, &f);
                    if (consider(s, sp[k].p, sp[k].q, K.key8[sp[k].p], K.key8[sp[k].q], c, f, inc)) {
                        // thread 0 appends its own admissions here (at most four)
                        const unsigned idx = atomicAdd(&st->nC, 1u);
                        if (idx < st->capC) P.C[idx] = make_uint4((unsigned)s, sp[k].p, sp[k].q, 0u);
                        else atomicOr(&st->err, ERR_C_FULL);
                    }
                }
            }
        } else {
            // C scan: entries untouched this round keep their counts during this launch
            const unsigned nC = st->nC_base;
            const unsigned stride = (gridDim.x - cell_blocks) * blockDim.x;
            for (unsigned i = g - cell_blocks * blockDim.x; i < nC; i += stride) {
                const uint4 e = P.C[i];
                const unsigned p = e.y, q = e.z;
                const unsigned f = P.flag[e.x];
                const long long c = P.cnt[e.x];
                const unsigned long long ka = K.key8[p], kb = K.key8[q];
                bool touched = false;
                if (q == a || q == nw) touched = LR[2 * (size_t)p] != 0;
                if (!touched && (p == b || p == nw)) touched = LR[2 * (size_t)q + 1] != 0;
                if (touched || !(f & kPresent)) continue;
                const Cand cand{c, ka, kb, e.x, p, q};
                if (cand_better(cand, best, K.pool, K.off, K.len)) best = cand;
            }
        }
        const unsigned idx = wave_append(add, &st->nC);
        if (add) {
            if (idx < st->capC) P.C[idx] = add_e;
            else atomicOr(&st->err, ERR_C_FULL);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const Cand oc = shfl_xor_cand(best, o);
        if (cand_better(oc, best, K.pool, K.off, K.len)) best = oc;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sw[w] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (cand_better(sw[k], best, K.pool, K.off, K.len)) best = sw[k];
        part[blockIdx.x] = Partial{best.cnt, best.ka, best.kb, best.slot, best.a, best.b, 0};
        if (blockIdx.x == 0 && !st->halt) {
            // finish the round: the new token enters the dedupe map; round/ntok advance (only
            // k_merge reads these, in the next launch)
            const unsigned nw = st->cur_new;
            if (st->new_is_new) {
                const unsigned long long h = K.hash[nw];
                unsigned s = (unsigned)mix64(h) & K.map_mask;
                while (K.map[s] != 0) s = (s + 1) & K.map_mask;
                K.map[s] = map_entry(h, nw);
            }
            st->round = st->cur_round + 1;
            st->ntok = st->cur_ntok;
        }
    }
}

// ------------------------------------------------------------------ argmax over C (rebuild)
// After the host re-thresholds C: per-block partials of the argmax over all of C.
__global__ void __launch_bounds__(256) k_argmax(RoundState* __restrict__ st, PairsDev P, ToksDev K,
                                                Partial* __restrict__ part) {
    __shared__ Cand sw[4];
    Cand best = cand_none();
    const unsigned nC = st->nC;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < nC; i += gridDim.x * blockDim.x) {
        const uint4 e = P.C[i];
        const unsigned f = P.flag[e.x];
        const long long c = P.cnt[e.x];
        const unsigned long long ka = K.key8[e.y], kb = K.key8[e.z];
        if (!(f & kPresent)) continue;
        const Cand x{c, ka, kb, e.x, e.y, e.z};
        if (cand_better(x, best, K.pool, K.off, K.len)) best = x;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const Cand oc = shfl_xor_cand(best, o);
        if (cand_better(oc, best, K.pool, K.off, K.len)) best = oc;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sw[w] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k)
            if (cand_better(sw[k], best, K.pool, K.off, K.len)) best = sw[k];
        part[blockIdx.x] = Partial{best.cnt, best.ka, best.kb, best.slot, best.a, best.b, 0};
    }
}

}  // namespace

}  // namespace bpe
