// Merge loop, batched rounds: the rewrite of a trip's batch (merge_word_batch, merge_body,
// k_merge_batch) and the fused select + merge kernel k_trip.
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include "train_select.h"

namespace bpe {

namespace {

// the slot word of class C addressed directly, every member applied in order.  claim: the word
// (global slot index f) may be on several members' lists; the first thread to claim it rewrites
// it.  The word is loaded before the claim: only the claimant writes it during this batch.
template <class TokT, int C>
__device__ __forceinline__ void merge_word_batch(const SlotCls<TokT>& S, unsigned i, const Batch& B,
                                                 unsigned long long* LRt, size_t lr_member,
                                                 unsigned* lds, bool narrow, const LdsU32* sm_a,
                                                 const LdsU32* sm_b, const LdsU32* sm_n, const LdsU8* pm, bool use_pm,
                                                 unsigned& singles, LdsU32* bm, unsigned tbw, unsigned mark_from,
                                                 uint32_t* tags = nullptr, unsigned f = 0) {
    constexpr int W = slot_w(C);
    constexpr int V = W * (int)sizeof(TokT) / 16;
    TokT* s = S.slot + (size_t)i * W;
    uint4 r[V];
#pragma unroll
    for (int v = 0; v < V; ++v) r[v] = reinterpret_cast<const uint4*>(s)[v];
    // the count: issued with the slot in a full scan (most words hit early); in list mode, where
    // most entries miss, only on a hit, beside the claim (one random line less per missing entry,
    // and the claim's round trip covers the load)
    unsigned long long c = 0;
    if (!tags) c = S.cnt[i];
    TokT e[W];
    __builtin_memcpy(e, r, sizeof(e));
    // the members this word holds: no member's b is another's a and the new tokens are fresh, so
    // a rewrite neither makes nor breaks another member's pair and the original word decides
    unsigned hits = 0;
    if (use_pm && W <= 32) {   // each pair of the word looked up in the batch's pair table, eight
        // lookups in flight at a time (the 64-id class, rare, compares with every member)
        const uint32_t len = (uint32_t)e[0];
#pragma unroll
        for (int q0 = 1; q0 + 1 < W; q0 += 8) {
            unsigned v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u;
                v[u] = q + 1 < W ? (unsigned)pm[pair_h12((unsigned)e[q + 1 < W ? q : 1], (unsigned)e[q + 1 < W ? q + 1 : 1])] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u;
                if (q + 1 < W && (uint32_t)q < len && v[u]) {
                    const unsigned x = (unsigned)e[q + 1 < W ? q : 1], y = (unsigned)e[q + 1 < W ? q + 1 : 1];
                    if (v[u] != 0xFFu) {
                        const unsigned j = v[u] - 1;
                        hits |= (unsigned)((x == sm_a[j]) & (y == sm_b[j])) << j;
                    } else {   // two members share the slot
                        for (int j = 0; j < B.k; ++j) hits |= (unsigned)((x == sm_a[j]) & (y == sm_b[j])) << j;
                    }
                }
            }
        }
    } else {
        for (int j = 0; j < B.k; ++j) {
            const TokT ta = (TokT)sm_a[j], tb = (TokT)sm_b[j];
            bool hit = false;
#pragma unroll
            for (int q = 1; q + 1 < W; ++q) hit |= (e[q] == ta) & (e[q + 1] == tb);
            hits |= (unsigned)hit << j;
        }
    }
    // claimed only on a hit (most list entries miss: no atomic for them).  A word rewritten under
    // another thread's claim was loaded after that claim, so its copy here, torn or not, ends in a
    // failed claim or in no hit: only the claimant ever writes it.
    if (!hits) return;
    if (tags) c = S.cnt[i];
    if (tags && atomicMax(&tags[f], B.batch_id) >= B.batch_id) return;
    if (W <= kRegRewriteMaxW) {   // every member in registers, one compacting store
        const auto sink_of = [&](int j) {
            return DeltaSinkN<kLdsB>{LRt + (size_t)j * lr_member, (LdsU32*)(lds + 2 * kLdsB * j), bm + j * tbw,
                                     mark_from, narrow};
        };
        const uint32_t nl = rewrite_slot_members(e, s, hits, sm_a, sm_b, sm_n, c, sink_of);
        singles += nl < 2;
        return;
    }
    bool first = true;
    while (hits) {
        const int j = __builtin_ctz(hits);
        hits &= hits - 1;
        if (!first) {   // a second member: the word as rewritten (this thread's own stores)
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = reinterpret_cast<const uint4*>(s)[v];
            __builtin_memcpy(e, r, sizeof(e));
        }
        first = false;
        const DeltaSinkN<kLdsB> D{LRt + (size_t)j * lr_member, (LdsU32*)(lds + 2 * kLdsB * j), bm + j * tbw,
                                  mark_from, narrow};
        const uint32_t nl = rewrite_slot(e, s, (TokT)sm_a[j], (TokT)sm_b[j], (TokT)sm_n[j], c, D);
        if (nl < 2) { ++singles; break; }
    }
}

// The merge-apply rewrite of a trip's batch B (the batch record in memory for k_merge_batch, the
// workgroup's own LDS copy in k_trip).  l_lr: the workgroup's LDS-summed cells (2 kLdsB per member).
template <class TokT>
__device__ __forceinline__ void merge_body(RoundState* __restrict__ st, const Batch& B, PairsDev P, ToksDev K,
                                           WordsDev<TokT> W, IndexDev X, unsigned long long* __restrict__ LRbase,
                                           size_t lr_member, size_t lr_parity, uint32_t* __restrict__ tags,
                                           const CellMarks CM, unsigned* l_lr) {
    __shared__ unsigned s_ma[kMaxBatch], s_mb[kMaxBatch], s_mn[kMaxBatch];   // the members' tokens
    __shared__ unsigned s_bm[kMaxBatch * kTBMax];   // the members' touched-block bitmaps (CellMarks)
    __shared__ unsigned s_pre[kMaxBatch + 1], s_lbeg[kMaxBatch];   // list prefix sums, list starts
    __shared__ unsigned s_pm[kPairSlots / 4];   // the batch's pair table (bytes; kPairFilterK)
    const int tid = threadIdx.x;
    // every field the prologue needs in one round trip (none depends on another)
    const int stop = B.stop, k = B.k, b_trip = B.trip, b_ntok = B.ntok, b_prev_k = B.prev_k,
              b_prev_sparse = B.prev_sparse;
    const unsigned idle_from = B.idle_from;
    // 32-bit LDS cells hold every member's sums (run-time test knob BPE355_LDS_CELLS=0: every cell
    // global, the path of a batch whose P1 count reaches 2^32)
    const bool narrow = B.m[0].cnt < st->narrow_limit;
    unsigned ma = 0, mb = 0, mn = 0, mlb = 0, mpre = 0;
    if (tid < kMaxBatch) { ma = B.m[tid].a; mb = B.m[tid].b; mn = B.m[tid].nw; mlb = B.m[tid].list_beg; }
    if (tid <= kMaxBatch) mpre = B.list_pre[tid];
    if (stop) return;
    const unsigned tbw = CM.tbw;
    const unsigned mark_from = tbw ? 2 * CM.dense_tok : ~0u;
    // the previous trip's cells (the other parity, read by its apply) are cleared here, spread
    // over the whole grid: workgroups without words do their share at once, the others after
    // their flush, so the stores never wait in front of a rewrite's loads.  With marks: the dense
    // token prefix, the blocks the previous apply listed (CM.tbc), and that parity's bitmaps
    auto clear_prev = [&]() {
        unsigned long long* LRo = LRbase + (size_t)((b_trip + 1) & 1) * lr_parity;
        const unsigned S = gridDim.x * blockDim.x, g = blockIdx.x * blockDim.x + tid;
        const unsigned pk = (unsigned)b_prev_k;
        unsigned* TBo = CM.tb + (size_t)((b_trip + 1) & 1) * kTBRep * kMaxBatch * tbw;
        if (tbw)   // that parity's bitmaps (the marks its merge made, whatever its apply did with them)
            for (unsigned q = g; q < kTBRep * kMaxBatch * tbw; q += S) TBo[q] = 0u;
        if (!tbw || !b_prev_sparse) {   // the previous apply scanned every cell: clear every cell
            const unsigned nprev = (unsigned)b_ntok;   // 16-byte cell pairs per member
            for (unsigned q = g; q < pk * nprev; q += S)
                *reinterpret_cast<uint4*>(&LRo[(size_t)(q / nprev) * lr_member + 2 * (q % nprev)]) = make_uint4(0, 0, 0, 0);
            return;
        }
        const unsigned nd2 = min(CM.dense_tok, (unsigned)b_ntok);   // 16-byte cell pairs per member
        for (unsigned q = g; q < pk * nd2; q += S)
            *reinterpret_cast<uint4*>(&LRo[(size_t)(q / nd2) * lr_member + 2 * (q % nd2)]) = make_uint4(0, 0, 0, 0);
        const unsigned nbk = 32 * tbw;   // blocks per member
        for (unsigned q = g; q < pk * nbk; q += S) {
            const unsigned j = q / nbk, blk = q % nbk;
            if ((CM.tbc[j * tbw + (blk >> 5)] >> (blk & 31)) & 1u) {
                uint4* c = reinterpret_cast<uint4*>(&LRo[(size_t)j * lr_member + 64 * (size_t)blk]);
#pragma unroll 8
                for (int u = 0; u < 32; ++u) c[u] = make_uint4(0, 0, 0, 0);
            }
        }
    };
    // Member j's pop and new-token registration (nothing in this launch reads them: the apply
    // and the next trip do) go to the first k workgroups without words when there are enough of
    // them, else to workgroups 0..k-1 after their rewrite: either way no rewrite waits behind the
    // registration's chain of dependent loads (the token bytes of a and b)
    const unsigned gl = min(gridDim.x, W.lblk0);   // the slot-class blocks that exist
    const unsigned busy = idle_from == ~0u ? gl : min(gl, (idle_from + blockDim.x - 1) / blockDim.x);
    const unsigned reg0 = busy + (unsigned)k <= gl ? busy : 0u;   // (the grid has >= kMaxBatch blocks)
    const int reg_j = (int)blockIdx.x - (int)reg0;
    auto register_member = [&]() {
        if (reg_j < 0 || reg_j >= k) return;
        const BatchMember& M = B.m[reg_j];
        if (tid == 0) {
            P.cnt[M.slot] = 0;                       // byte_pair_frequencies.pop(best_pair)
            atomicAnd(&P.flag[M.slot], ~kPresent);
            X.beg[M.nw] = M.cov_beg;
            X.len[M.nw] = M.cov_len;
        }
        if (M.isnew) {
            if (M.pool_off + M.ln <= st->pool_cap) {
                const unsigned la = K.len[M.a];
                for (unsigned i = tid; i < M.ln; i += blockDim.x) K.pool[M.pool_off + i] = concat_byte(K, M.a, la, M.b, i);
            } else if (tid == 0) {
                atomicOr(&st->err, ERR_POOL);
            }
            if (tid == 0) {
                K.off[M.nw] = M.pool_off; K.len[M.nw] = M.ln;
                K.hash[M.nw] = M.hash; K.pw[M.nw] = M.pw; K.key8[M.nw] = M.k8;
            }
        }
    };
    {   // list mode: workgroups past the listed words have no rewrite -- skip their LDS clear,
        // barriers and flush
        const unsigned bid = blockIdx.x;
        if (bid >= busy && bid < gl) {
            register_member();
            clear_prev();
            if (tid == 0) probe_done(st, &st->probe_merge_done, b_trip, 14);
            return;
        }
    }
    if (tid < k) {
        s_ma[tid] = ma; s_mb[tid] = mb; s_mn[tid] = mn;
        s_lbeg[tid] = mlb;
    }
    if (tid <= k) s_pre[tid] = mpre;
    if (blockIdx.x == 0 && tid == 0) probe_stamp(st, B.trip, 5);
    for (unsigned q = tid; q < 2 * kLdsB * (unsigned)k; q += blockDim.x) l_lr[q] = 0;
    for (unsigned q = tid; q < tbw * (unsigned)k; q += blockDim.x) s_bm[q] = 0;
    LdsU32* lbm = (LdsU32*)s_bm;
    unsigned long long* LRt = LRbase + (size_t)(B.trip & 1) * lr_parity;   // member j at + j * lr_member
    const bool use_pm = k >= kPairFilterK;   // (uniform)
    if (use_pm)
        for (unsigned q = tid; q < kPairSlots / 4; q += blockDim.x) s_pm[q] = 0;

    __syncthreads();   // l_lr cleared
    if (use_pm) {   // member j's pair -> slot: j + 1, or 0xFF where two members share a slot
        if (tid < 64) {
            const bool m = tid < k;
            const unsigned h = pair_h12(ma, mb);
            bool coll = false;
#pragma unroll
            for (int j = 0; j < kMaxBatch; ++j) {
                const int hj = __shfl((int)h, j);   // (every lane active: lane j supplies its slot)
                coll |= j < k && j != tid && hj == (int)h;
            }
            if (m) reinterpret_cast<uint8_t*>(s_pm)[h] = coll ? (uint8_t)0xFFu : (uint8_t)(tid + 1);
        }
        __syncthreads();
    }
    const LdsU8* pmp = (const LdsU8*)s_pm;
    if (blockIdx.x == 0 && tid == 0) probe_stamp(st, B.trip, 6);

    unsigned singles = 0;
    const unsigned bid = blockIdx.x;
    // the host may launch fewer blocks than the slot-class layout has (short posting lists late
    // in training): every loop below strides over the nb blocks that exist
    const unsigned nb = gridDim.x < W.lblk0 ? gridDim.x : W.lblk0;
    if (k == 1) {
        // one member: the per-round rewrite (index list or a scan of every slot)
        const BatchMember& M = B.m[0];
        const TokT ta = (TokT)M.a, tb = (TokT)M.b, tn = (TokT)M.nw;
        const DeltaSinkN<kLdsB> D{LRt, (LdsU32*)l_lr, lbm, mark_from, narrow};
        if (M.use_list && bid < nb) {
            const uint32_t* L = X.list + M.list_beg;
            for (unsigned i = bid * blockDim.x + tid; i < M.list_len; i += nb * blockDim.x) {
                const unsigned f = L[i];
                if (f < W.off[1]) merge_one<TokT, 0>(W.c[0], f, ta, tb, tn, D, singles);
                else if (f < W.off[2]) merge_one<TokT, 1>(W.c[1], f - W.off[1], ta, tb, tn, D, singles);
                else if (f < W.off[3]) merge_one<TokT, 2>(W.c[2], f - W.off[2], ta, tb, tn, D, singles);
                else merge_one<TokT, 3>(W.c[3], f - W.off[3], ta, tb, tn, D, singles);
            }
        } else if (!M.use_list) {
            for (unsigned bb = bid; bb < W.lblk0; bb += nb) {
                if (bb < W.c[1].blk0) {
                    if (bb < W.c[0].blk0 + W.c[0].nblk)
                        scan_class<TokT, 0>(W.c[0], bb - W.c[0].blk0, ta, tb, tn, D, singles);
                } else if (bb < W.c[2].blk0) {
                    scan_class<TokT, 1>(W.c[1], bb - W.c[1].blk0, ta, tb, tn, D, singles);
                } else if (bb < W.c[3].blk0) {
                    scan_class<TokT, 2>(W.c[2], bb - W.c[2].blk0, ta, tb, tn, D, singles);
                } else {
                    scan_class<TokT, 3>(W.c[3], bb - W.c[3].blk0, ta, tb, tn, D, singles);
                }
            }
        }
    } else if (bid < nb) {
        // several members: every word that can contain one of them, once, all members in order
        if (B.full_scan) {
            const unsigned total = W.off[kNumCls];
            for (unsigned f = bid * blockDim.x + tid; f < total; f += nb * blockDim.x) {
                if (f < W.off[1]) merge_word_batch<TokT, 0>(W.c[0], f,  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from);
                else if (f < W.off[2]) merge_word_batch<TokT, 1>(W.c[1], f - W.off[1],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from);
                else if (f < W.off[3]) merge_word_batch<TokT, 2>(W.c[2], f - W.off[2],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from);
                else merge_word_batch<TokT, 3>(W.c[3], f - W.off[3],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from);
            }
        } else {
            const unsigned total = B.list_pre[k];
            for (unsigned i = bid * blockDim.x + tid; i < total; i += nb * blockDim.x) {
                int j = 0;
                // the member whose list holds entry i: binary search of the LDS prefix sums, steps
                // from the largest power of two below kMaxBatch (any cap, not only powers of two)
                for (int step = kListTopStep; step > 0; step >>= 1)
                    if (j + step < k && i >= s_pre[j + step]) j += step;
                const unsigned f = X.list[s_lbeg[j] + (i - s_pre[j])];
                // a word on several members' lists is rewritten by the first thread to claim it
                if (f < W.off[1]) merge_word_batch<TokT, 0>(W.c[0], f,  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from, tags, f);
                else if (f < W.off[2]) merge_word_batch<TokT, 1>(W.c[1], f - W.off[1],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from, tags, f);
                else if (f < W.off[3]) merge_word_batch<TokT, 2>(W.c[2], f - W.off[2],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from, tags, f);
                else merge_word_batch<TokT, 3>(W.c[3], f - W.off[3],  B, LRt, lr_member, l_lr, narrow, (const LdsU32*)s_ma, (const LdsU32*)s_mb, (const LdsU32*)s_mn, pmp, use_pm, singles, lbm, tbw, mark_from, tags, f);
            }
        }
    }
    if (bid >= W.lblk0 && bid < W.lblk0 + W.lnblk) {   // long words: every member in order
        for (unsigned i = (bid - W.lblk0) * blockDim.x + tid; i < W.ln; i += W.lnblk * blockDim.x) {
            uint32_t len = W.llen[i];
            if (len < 2) continue;
            TokT* t = W.ltok + W.lbeg[i];
            for (int j = 0; j < k && len >= 2; ++j) {
                const TokT ta = (TokT)B.m[j].a, tb = (TokT)B.m[j].b;
                bool hit = false;
                for (uint32_t q = 0; q + 1 < len && !hit; ++q) hit = (t[q] == ta) & (t[q + 1] == tb);
                if (!hit) continue;
                const DeltaSinkN<kLdsB> D{LRt + (size_t)j * lr_member, (LdsU32*)(l_lr + 2 * kLdsB * j), lbm + j * tbw,
                                          mark_from, narrow};
                len = rewrite_word(t, len, ta, tb, (TokT)B.m[j].nw, W.lcnt[i], D, false);
                W.llen[i] = len;
                singles += (len < 2);
            }
        }
    }
    singles = wave_sum(singles);   // words that became one token (rare: no contention)
    // (the apply adds them to n_single, which this trip's select phase reads in every workgroup)
    if ((tid & 63) == 0 && singles) atomicAdd(&st->n_single_new, singles);
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) probe_stamp(st, B.trip, 7);
    for (unsigned q = tid; q < 2 * kLdsB * (unsigned)k; q += blockDim.x) {
        const unsigned v = l_lr[q];
        if (v) atomicAdd(&LRt[(size_t)(q / (2 * kLdsB)) * lr_member + q % (2 * kLdsB)], (unsigned long long)v);
    }
    if (tbw) {   // the touched blocks, into this workgroup's replica of this parity's bitmaps
        unsigned* TBt = CM.tb + ((size_t)(B.trip & 1) * kTBRep + blockIdx.x % kTBRep) * kMaxBatch * tbw;
        for (unsigned q = tid; q < tbw * (unsigned)k; q += blockDim.x) {
            const unsigned v = s_bm[q];
            if (v) atomicOr(&TBt[q], v);
        }
    }
    if (blockIdx.x == 0 && tid == 0) probe_stamp(st, B.trip, 8);
    clear_prev();
    register_member();
    if (BPE355_PROBE_CODE && st->probe) {
        __syncthreads();
        if (tid == 0) probe_done(st, &st->probe_merge_done, B.trip, 14);
    }
}

// the rewrite of the batch k_select decided (BPE355_FOLD=0)
constexpr int kMergeWaves = 4;   // waves per EU the u16 instantiation is compiled for
template <class TokT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(TokT) == 2 ? kMergeWaves : 2))) k_merge_batch(RoundState* __restrict__ st, const Batch* __restrict__ bt,
                                                     PairsDev P, ToksDev K, WordsDev<TokT> W, IndexDev X,
                                                     unsigned long long* __restrict__ LRbase, size_t lr_member,
                                                     size_t lr_parity, uint32_t* __restrict__ tags, CellMarks CM) {
    __shared__ unsigned l_lr[2 * kLdsB * kMaxBatch];
    merge_body<TokT>(st, *bt, P, K, W, X, LRbase, lr_member, lr_parity, tags, CM, l_lr);
}

// One trip's select and merge in ONE launch.  Every workgroup decides the
// batch itself -- the decision is a function of state that nothing in this launch changes
// (select_core) -- so no workgroup waits for another and the select's kernel boundary is gone.
// Block 0 also publishes the batch record the apply reads.  Measured on the bench config it is
// no faster than k_select + k_merge_batch (257.4-258.3 vs 255.4 ms of merges): the boundary it
// saves (2-4 us) is paid back by the decision's own loads, which every workgroup repeats (the
// apply's 24 KB of partials arrive 1.3 us later with 1024 readers than with one), so it is the
// BPE355_FOLD=1 option, not the default.  The select's LDS and the
// rewrite's LDS-summed cells share one union: the cells are cleared after the decision.
template <class TokT>
__global__ void __launch_bounds__(kTripThreads) k_trip(RoundState* __restrict__ st, BatchState* __restrict__ bs,
                                              PairsDev P, ToksDev K, WordsDev<TokT> W, IndexDev X,
                                              Batch* __restrict__ bt, const Partial* __restrict__ part,
                                              const Partial* __restrict__ lists, SelOut O,
                                              unsigned long long* __restrict__ LRbase, size_t lr_member,
                                              size_t lr_parity, uint32_t* __restrict__ tags, CellMarks CM) {
    __shared__ union TripLds {
        SelLds sel;
        unsigned lr[2 * kLdsB * kMaxBatch];
    } u;
    __shared__ Batch s_b;
    const bool pub = blockIdx.x == 0;
    select_core<kTripThreads>(st, bs, K, X, part, lists, s_b, u.sel, O, pub);
    __syncthreads();
    if (pub) {   // the apply's copy of the decision
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&s_b);
        uint32_t* dst = reinterpret_cast<uint32_t*>(bt);
        for (unsigned i = threadIdx.x; i < (unsigned)(sizeof(Batch) / 4); i += blockDim.x) dst[i] = src[i];
    }
    if (s_b.stop) return;
    merge_body<TokT>(st, s_b, P, K, W, X, LRbase, lr_member, lr_parity, tags, CM, u.lr);
}

}  // namespace

}  // namespace bpe
