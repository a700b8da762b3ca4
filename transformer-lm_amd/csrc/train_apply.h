// Merge loop, batched rounds: k_apply_batch (the trip's deltas onto the pair table, the next
// trip's candidates).
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include "train_merge.h"

namespace bpe {

namespace {

// Apply the trip's deltas and list the next trip's candidates.  Items:
//   v < k * 4 * ntb        member j = v / (4 ntb), token x, op as in k_apply_argmax; its key has
//                          ONE updater unless x is one of the batch's tokens S = {a_j, b_j, new_j};
//   next |S|^2 items       every key with both tokens in S: one item sums all the members'
//                          contributions to it;
//   next nC_base items     C entries: untouched ones keep their counts during the apply, touched
//                          ones are evaluated by their updater (final count).
// Every present key >= T among them is a candidate; each workgroup writes its exact top-kTopM
// (sorted) to part[blockIdx.x * kTopM ...] and k_select merges the lists.  scan_only: the C
// entries alone (after a rebuild of C).
constexpr unsigned kBatchApplyItems = 2;   // items per thread per pass of k_apply_batch
constexpr unsigned kApplyBatchThreads = 256;
constexpr unsigned kApplyCLds = 256;
constexpr unsigned kSFilterWords = 128;   // C admissions a workgroup stages in LDS (more: direct appends)
__global__ void __launch_bounds__(kApplyBatchThreads) k_apply_batch(RoundState* __restrict__ st,
                                                                    BatchState* __restrict__ bs,
                                                                    const Batch* __restrict__ bt, PairsDev P, ToksDev K,
                                                                    unsigned long long* __restrict__ LRbase,
                                                                    size_t lr_member, size_t lr_parity, unsigned ntb,
                                                                    Partial* __restrict__ part,
                                                                    Partial* __restrict__ list, int scan_only,
                                                                    CellMarks CM, int sparse_hint) {
    __shared__ unsigned s_tok[3 * kMaxBatch];
    __shared__ unsigned s_tw[kMaxBatch * kTBMax];   // touched-block bitmaps (the replicas' OR)
    __shared__ unsigned short s_tl[kTLCap];         // touched blocks past the dense prefix: j << 11 | block
    __shared__ unsigned s_wsum[kApplyBatchThreads / 64];
    __shared__ unsigned s_role[3 * kMaxBatch];   // S entry: members' mask << 3 | role (1 a, 2 b, 4 new)
    __shared__ unsigned s_grp[2 * kMaxBatch];    // member j's a group (2j) and b group (2j + 1)
    __shared__ unsigned s_filt[kSFilterWords];   // bit (x mod 4096): x may be in S
    __shared__ int s_ns;
    __shared__ Cand s_wave[kApplyBatchThreads / 64];
    __shared__ Partial s_lst[kListCap];
    __shared__ uint4 s_cadd[kApplyCLds];
    __shared__ unsigned s_nl, s_nc, s_lbase, s_cbase, s_ins;
    const Batch& B = *bt;
    const int tid = threadIdx.x;
    // every field the prologue needs in one round trip (none depends on another); the batch is
    // valid memory even when stale (scan_only), so its loads need no guard
    static_assert(offsetof(BatchMember, b) == 4 && offsetof(BatchMember, nw) == 8, "a, b, nw adjacent");
    const int b_stop = B.stop, b_k = B.k, b_trip = B.trip, b_ntok = B.ntok;
    const unsigned b_fresh = B.n_fresh, b_nC = B.nC_base;
    const long long b_T2 = B.T2next;
    const long long T = st->T, T2bs = bs->T2;
    const int bs_trip = bs->trip;
    const unsigned st_nC = st->nC;   // scan_only: no admissions during the scan, so stable
    const unsigned t_raw = tid < 3 * kMaxBatch ? reinterpret_cast<const unsigned*>(&B.m[tid / 3])[tid % 3] : ~0u;
    static_assert(offsetof(BatchMember, gb) == offsetof(BatchMember, ga) + 4, "ga, gb adjacent");
    const unsigned g_raw = tid < 3 * kMaxBatch && tid % 3 < 2 ? (&B.m[tid / 3].ga)[tid % 3] : 0u;
    // touched-block bitmaps of both parities (CellMarks), issued with the batch record's loads
    // rather than behind them (the parity is the batch's); kTBW words per thread
    constexpr unsigned kTBW = (kMaxBatch * kTBMax + kApplyBatchThreads - 1) / kApplyBatchThreads;
    unsigned t2[2][kTBW];
    {
        const bool want = sparse_hint && !scan_only && CM.tbw != 0;
#pragma unroll
        for (unsigned pty = 0; pty < 2; ++pty)
#pragma unroll
            for (unsigned u = 0; u < kTBW; ++u) {
                const unsigned q = tid * kTBW + u;
                unsigned v = 0;
                if (want && q < kMaxBatch * CM.tbw)
#pragma unroll
                    for (unsigned r = 0; r < kTBRep; ++r)
                        v |= CM.tb[((size_t)pty * kTBRep + r) * kMaxBatch * CM.tbw + q];
                t2[pty][u] = v;
            }
    }
    if (!scan_only && b_stop) {   // no trip: part[] and the list keep what the next select reads
        if (b_stop > 0 && blockIdx.x == 0 && tid == 0) st->halt = b_stop;   // the select's halt
        return;
    }
    // the threshold of the list this apply fills (the trip's decision, or after a rebuild the
    // last one), and which of the two lists: the next trip's parity
    const long long T2raw = scan_only ? T2bs : b_T2;
    const unsigned lpar = (unsigned)(scan_only ? bs_trip : b_trip + 1) & 1u;
    list += (size_t)lpar * kListCap;
    const int k = scan_only ? 0 : b_k;
    const bool pw0 = !scan_only && blockIdx.x == 0 && tid == 0;
    if (pw0) probe_stamp(st, b_trip, 9);
    // touched blocks (CellMarks): listed from cm.sparse_from tokens on (below, the dense scan of
    // every cell is cheaper than building the list)
    const unsigned tbw = CM.tbw;
    const unsigned ntb_all = scan_only ? ntb : min(ntb, (unsigned)b_ntok + b_fresh);
    const bool sparse = sparse_hint && !scan_only && tbw != 0 && ntb_all > CM.sparse_from;   // (uniform)
    unsigned tw[kTBW];
#pragma unroll
    for (unsigned u = 0; u < kTBW; ++u)
        tw[u] = sparse && tid * kTBW + u < (unsigned)k * tbw ? t2[b_trip & 1][u] : 0u;
    if (tid < 64) {   // wave 0: S deduplicated (a == b is possible only when k == 1), lane i = entry i
        static_assert(3 * kMaxBatch <= 64, "S fits one wave");
        const int i = tid;
        const bool have = i < 3 * k;
        const unsigned ti = have ? t_raw : ~0u;
        // For k > 1 a token has one role: no member's b is another's a, a != b, and the new tokens
        // are fresh ids (select_core's rule); an a (a b) several members share is kept once, by
        // the group's first member, with the group's mask.  For k == 1 only a == b can repeat (a
        // new token's bytes are longer than a's and b's), so no general dedupe pass is needed.
        unsigned roles = 1u << (i % 3);
        const unsigned gm = i % 3 == 2 ? 1u << (i / 3) : g_raw;   // the members behind this entry
        bool dup = false;
        if (k == 1 && __builtin_amdgcn_readlane((int)ti, 0) == __builtin_amdgcn_readlane((int)ti, 1)) {
            if (i == 0) roles = 3u;   // a == b: one entry, both roles
            dup = i == 1;
        }
        if (have && i % 3 < 2) s_grp[2 * (i / 3) + i % 3] = gm;
        const bool keep = have && !dup && gm != 0;
        const unsigned long long km = __ballot(keep);
        for (unsigned w = i; w < kSFilterWords; w += 64) s_filt[w] = 0;
        if (keep) {
            const unsigned pos = __builtin_amdgcn_mbcnt_hi((unsigned)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)km, 0u));
            s_tok[pos] = ti;
            s_role[pos] = gm << 3 | roles;
            atomicOr(&s_filt[(ti >> 5) % kSFilterWords], 1u << (ti & 31));
        }
        if (i == 0) {
            s_ns = __popcll(km);
            s_nl = 0;
            s_nc = 0;
            s_ins = 0;
        }
    }
    __syncthreads();
    const int ns = s_ns;
    const unsigned long long* LRc = LRbase + (size_t)(b_trip & 1) * lr_parity;
    ntb = ntb_all;   // token ids after this trip
    const unsigned per_member = 4 * ntb;
    // the cell items: every (member, token, op) densely, or (sparse) the dense token prefix of every
    // member plus the touched blocks past it, 128 items (32 tokens x 4 ops) per block
    const unsigned nD = CM.dense_tok / 32;   // dense-prefix blocks per member
    unsigned n_cell = (unsigned)k * per_member;
    bool listed = false;
    if (sparse) {
        // a token group's first member updates (x, a) / (b, y) for the whole group from the
        // group's summed cells: its blocks must cover every group member's
#pragma unroll
        for (unsigned u = 0; u < kTBW; ++u) {
            const unsigned q = tid * kTBW + u;
            if (q < (unsigned)k * tbw) s_tw[q] = tw[u];
        }
        __syncthreads();
        // (from the members' own bitmaps only: every workgroup must list exactly the same blocks,
        // since the items are numbered across the grid -- a leader that is itself in another
        // leader's group must not pass on bits in an order that depends on timing)
        unsigned c = 0;
#pragma unroll
        for (unsigned u = 0; u < kTBW; ++u) {
            const unsigned q = tid * kTBW + u;
            if (q >= (unsigned)k * tbw) continue;
            const unsigned j = q / tbw, w = q % tbw;
            unsigned gm = (s_grp[2 * j] | s_grp[2 * j + 1]) & ~(1u << j);
            while (gm) {
                const unsigned m = (unsigned)__builtin_ctz(gm);
                gm &= gm - 1;
                tw[u] |= s_tw[m * tbw + w];
            }
            c += __popc(tw[u]);
        }
        // exclusive scan of the counts over the workgroup
        unsigned inc = c;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(inc, d);
            if ((tid & 63) >= d) inc += t;
        }
        if ((tid & 63) == 63) s_wsum[tid >> 6] = inc;
        __syncthreads();
        unsigned base = 0, T = 0;
        for (int w = 0; w < (int)(kApplyBatchThreads / 64); ++w) {
            const unsigned ws = s_wsum[w];
            base += w < (tid >> 6) ? ws : 0u;
            T += ws;
        }
        base += inc - c;
        if (T <= kTLCap) {
            listed = true;
#pragma unroll
            for (unsigned u = 0; u < kTBW; ++u) {
                unsigned v = tw[u];
                const unsigned q = tid * kTBW + u;
                while (v) {
                    const unsigned bit = (unsigned)__builtin_ctz(v);
                    v &= v - 1;
                    s_tl[base++] = (unsigned short)((q / tbw) << 11 | ((q % tbw) * 32 + bit));
                }
            }
            n_cell = ((unsigned)k * nD + T) * 128;
        }
        if (CM.sig) {   // (test knob) this workgroup's view: T and a hash of its bitmaps
            unsigned long long hsh = 0;
#pragma unroll
            for (unsigned u = 0; u < kTBW; ++u) hsh += (unsigned long long)tw[u] * (0x9E3779B97F4A7C15ull * (tid * kTBW + u + 1));
            for (int o = 32; o > 0; o >>= 1) hsh += __shfl_xor(hsh, o);
            if ((tid & 63) == 0) atomicAdd(&CM.sig[1 + blockIdx.x], hsh + ((unsigned long long)T << 48));
        }
        if (blockIdx.x == 0)   // for the next merge's clear
#pragma unroll
            for (unsigned u = 0; u < kTBW; ++u) {
                const unsigned q = tid * kTBW + u;
                if (q < (unsigned)k * tbw) CM.tbc[q] = tw[u];
            }
        __syncthreads();
    }
    // cell item v -> member j, token x, op (false: no such cell)
    auto cell_of = [&](unsigned v, unsigned& j, unsigned& x, unsigned& op) -> bool {
        if (!listed) {
            j = v / per_member;
            const unsigned r = v % per_member;
            x = r >> 2;
            op = r & 3;
            return true;
        }
        const unsigned slot = v >> 7, r = v & 127;
        unsigned blk;
        if (slot < (unsigned)k * nD) {
            j = slot / nD;
            blk = slot % nD;
        } else {
            const unsigned e = s_tl[slot - (unsigned)k * nD];
            j = e >> 11;
            blk = e & 2047u;
        }
        x = blk * 32 + (r >> 2);
        op = r & 3;
        return x < ntb;
    };
    const unsigned n_sp = (unsigned)(ns * ns);
    const unsigned nC0 = scan_only ? st_nC : b_nC;
    const unsigned n_items = n_cell + n_sp + nC0;
    const unsigned g = blockIdx.x * blockDim.x + tid;
    const unsigned S = gridDim.x * blockDim.x;
    // (the previous trip's cells were cleared by this trip's merge)
    if (pw0) probe_stamp(st, b_trip, 10);
    auto find_S = [&](unsigned x) -> int {   // x's entry in S, or -1
        if (!((s_filt[(x >> 5) % kSFilterWords] >> (x & 31)) & 1u)) return -1;
        int r = -1;
        for (int u = 0; u < ns; ++u) r = s_tok[u] == x ? u : r;
        return r;
    };
    auto in_S = [&](unsigned x) { return find_S(x) >= 0; };
    // the cells at index ci of the members in mask (one load unless members share the token)
    auto cell_sum = [&](unsigned mask, size_t ci) -> unsigned long long {
        unsigned long long t = 0;
        while (mask) {
            const unsigned j = (unsigned)__builtin_ctz(mask);
            mask &= mask - 1;
            t += LRc[(size_t)j * lr_member + ci];
        }
        return t;
    };
    const long long T2 = T2raw < T ? T : T2raw;
    Cand best = cand_none();   // this thread's best candidate (exact argmax)
    unsigned n_ins = 0;        // pair-table keys this thread inserted
    // a candidate for the list (>= T2) and for this thread's best
    auto offer = [&](const Cand& c) {
        if (cand_better(c, best, K.pool, K.off, K.len)) best = c;
        const bool listed = c.cnt != LLONG_MIN && c.cnt >= T2;
        const unsigned li = wave_append(listed, &s_nl);   // one LDS atomic per wave
        if (listed && li < kListCap) s_lst[li] = Partial{c.cnt, c.ka, c.kb, c.slot, c.a, c.b, 0};
    };
    // an increment across T admits the key to C
    auto admit = [&](bool pred, size_t s, unsigned p, unsigned q) {
        const unsigned ci = wave_append(pred, &s_nc);
        if (!pred) return;
        if (ci < kApplyCLds) {
            s_cadd[ci] = make_uint4((unsigned)s, p, q, 0u);
        } else {
            const unsigned idx = atomicAdd(&st->nC, 1u);
            if (idx < st->capC) P.C[idx] = make_uint4((unsigned)s, p, q, 0u);
            else atomicOr(&st->err, ERR_C_FULL);
        }
    };
    // an updated key: a candidate if present and >= T
    auto updated = [&](size_t s, unsigned p, unsigned q, long long c, unsigned f, bool inc,
                       unsigned long long kp, unsigned long long kq) {
        if (s == ~(size_t)0 || !(f & kPresent) || c < T) return;
        offer(Cand{c, kp, kq, (unsigned)s, p, q});
        const bool adm = inc && !(f & kInC);
        if (adm) {   // (the address before the value: k_apply_batch's code depends on the order)
            unsigned* const fl = &P.flag[s];
            *fl = f | kInC;
        }
        admit(adm, s, p, q);
    };
    // step u of a pass takes items base + u * S + g: a wave's 64 items are contiguous (coalesced)
    // and its steps far apart, so the dense start of each member's cells (the byte tokens, which
    // neighbour everything) spreads over many waves instead of serialising in a few
    // item order: cells, S pairs, C entries (the C entries first was measured no faster:
    // profiles/r03/h_apply_c_first_ab.txt)
    for (unsigned base = 0; base < n_items; base += S * kBatchApplyItems) {
        // three stages over the thread's items, so that their dependent loads overlap instead of
        // chaining item after item: (1) each item's first load -- its cell, an S key's two cells, a
        // C entry; (2) each item's key and the loads it needs -- the key's home slot and both
        // tokens' prefixes (an update), or the slot state and the touched cells (a C entry);
        // (3) the updates and offers
        unsigned long long dv[kBatchApplyItems], dw[kBatchApplyItems];
        uint4 ce[kBatchApplyItems];
#pragma unroll
        for (unsigned u = 0; u < kBatchApplyItems; ++u) {
            const unsigned v = base + u * S + g;
            dv[u] = 0;
            dw[u] = 0;
            ce[u] = make_uint4(0, 0, 0, 0);
            unsigned j, x, op;
            if (v < n_cell) {
                if (!cell_of(v, j, x, op)) continue;
                const size_t ci = 2 * (size_t)x + (op >> 1);
                dv[u] = LRc[(size_t)j * lr_member + ci];
                if (!(op & 1)) {   // (x, a_j) or (b_j, x): one updater per token group
                    const unsigned gmask = s_grp[2 * j + (op >> 1)];
                    if (gmask != 1u << j) dv[u] = gmask ? cell_sum(gmask, ci) : 0ull;
                }
            } else if (v < n_cell + n_sp) {
                const unsigned sp = v - n_cell;
                const unsigned p = s_tok[sp / ns], q = s_tok[sp % ns];
                const unsigned rp = s_role[sp / ns], rq = s_role[sp % ns];
                // q's members see p on their left (cell 2p), p's see q on their right (2q + 1)
                if (rq & 5) dv[u] = cell_sum(rq >> 3, 2 * (size_t)p);
                if (rp & 6) dw[u] = cell_sum(rp >> 3, 2 * (size_t)q + 1);
            } else if (v < n_items) {
                ce[u] = P.C[v - n_cell - n_sp];
            }
        }
        unsigned ip[kBatchApplyItems], iq[kBatchApplyItems], how[kBatchApplyItems];   // how: 1 update, 2 inc, 4 C entry
        long long delta[kBatchApplyItems], hc[kBatchApplyItems];
        unsigned long long hk[kBatchApplyItems], kp[kBatchApplyItems], kq[kBatchApplyItems];
        unsigned hf[kBatchApplyItems];
        bool touched[kBatchApplyItems];
#pragma unroll
        for (unsigned u = 0; u < kBatchApplyItems; ++u) {
            const unsigned v = base + u * S + g;
            how[u] = 0; ip[u] = 0; iq[u] = 0; delta[u] = 0; touched[u] = false;
            hk[u] = 0; hc[u] = 0; hf[u] = 0; kp[u] = 0; kq[u] = 0;
            unsigned j, x, op;
            if (v < n_cell) {
                const long long d = cell_of(v, j, x, op) ? (long long)dv[u] : 0ll;
                if (d && !in_S(x)) {
                    const BatchMember& M = B.m[j];
                    ip[u] = op <= 1 ? x : (op == 2 ? M.b : M.nw);
                    iq[u] = op == 0 ? M.a : (op == 1 ? M.nw : x);
                    const bool inc = op & 1;
                    delta[u] = inc ? d : -d;
                    how[u] = 1 | (inc ? 2 : 0);
                }
            } else if (v < n_cell + n_sp) {
                const unsigned sp = v - n_cell;
                const unsigned rp = s_role[sp / ns], rq = s_role[sp % ns];
                const long long lq = (long long)dv[u], lp = (long long)dw[u];
                const bool popped = ((rp >> 3) & (rq >> 3)) != 0 && (rp & 1) && (rq & 2);
                long long inc = 0, dec = 0;
                if (rq & 1) dec += lq;
                if (rq & 4) inc += lq;
                if (rp & 2) dec += lp;
                if (rp & 4) inc += lp;
                if (!popped && (inc || dec)) {
                    ip[u] = s_tok[sp / ns];
                    iq[u] = s_tok[sp % ns];
                    delta[u] = inc - dec;
                    how[u] = 1 | (inc != 0 ? 2 : 0);
                }
            } else if (v < n_items) {
                const unsigned p = ce[u].y, q = ce[u].z;
                ip[u] = p;
                iq[u] = q;
                how[u] = 4;
                // does an item of this trip update the key?
                const int sp_ = find_S(p), sq_ = find_S(q);
                const unsigned rp = sp_ >= 0 ? s_role[sp_] : 0u, rq = sq_ >= 0 ? s_role[sq_] : 0u;
                const unsigned long long t1 = (rq & 5) ? cell_sum(rq >> 3, 2 * (size_t)p) : 0ull;
                const unsigned long long t2 = (rp & 6) ? cell_sum(rp >> 3, 2 * (size_t)q + 1) : 0ull;
                touched[u] = (t1 | t2) != 0;
                hf[u] = P.flag[ce[u].x];
                hc[u] = P.cnt[ce[u].x];
            }
            if (how[u] & 1) {   // the key's home slot: at load <= 1/2 it usually decides
                const size_t s0 = mix64(pair_key(ip[u], iq[u])) & P.mask;
                hk[u] = P.key[s0];
                hc[u] = P.cnt[s0];
                hf[u] = P.flag[s0];
            }
            if (how[u]) {
                kp[u] = K.key8[ip[u]];
                kq[u] = K.key8[iq[u]];
            }
        }
#pragma unroll
        for (unsigned u = 0; u < kBatchApplyItems; ++u) {
            if (how[u] & 1) {
                long long c;
                unsigned f;
                const size_t s = pair_update_from(P, st, ip[u], iq[u], delta[u], (how[u] & 2) != 0, hk[u], hc[u],
                                                  hf[u], &c, &f, n_ins);
                updated(s, ip[u], iq[u], c, f, (how[u] & 2) != 0, kp[u], kq[u]);
            } else if (how[u] & 4) {
                if (!touched[u] && (hf[u] & kPresent)) offer(Cand{hc[u], kp[u], kq[u], ce[u].x, ip[u], iq[u]});
            }
        }
    }
    if (pw0) probe_stamp(st, B.trip, 11);
    best = wave_best(best, K);
    n_ins = wave_sum(n_ins);
    if ((tid & 63) == 0 && n_ins) atomicAdd(&s_ins, n_ins);
    if ((tid & 63) == 0) s_wave[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (int)(kApplyBatchThreads / 64); ++w)
            if (cand_better(s_wave[w], best, K.pool, K.off, K.len)) best = s_wave[w];
        part[blockIdx.x] = Partial{best.cnt, best.ka, best.kb, best.slot, best.a, best.b, 0};
        // the workgroup's list entries and C admissions: one reservation each
        const unsigned nl = s_nl, nc = min(s_nc, kApplyCLds);
        s_lbase = nl ? atomicAdd(&bs->list_n[lpar], nl) : 0u;
        s_cbase = nc ? atomicAdd(&st->nC, nc) : 0u;
        if (s_ins) atomicAdd(&st->pair_used, (unsigned long long)s_ins);   // read by the next select
    }
    if (s_nl | s_nc) {   // (uniform: read after the barrier) only workgroups with entries wait
        __syncthreads();
        const unsigned nl = min(s_nl, kListCap), nc = min(s_nc, kApplyCLds);
        const unsigned lb = s_lbase, cb = s_cbase;
        if ((unsigned)tid < nl && lb + tid < kListCap) list[lb + tid] = s_lst[tid];
        for (unsigned i = tid; i < nc; i += blockDim.x) {
            if (cb + i < st->capC) P.C[cb + i] = s_cadd[i];
            else atomicOr(&st->err, ERR_C_FULL);
        }
    }
    if (pw0) probe_stamp(st, B.trip, 12);
    if (blockIdx.x == gridDim.x - 1 && tid < k && B.m[tid].isnew) {   // the new tokens enter the dedupe map
        const unsigned nw = B.m[tid].nw;
        const unsigned long long h = B.m[tid].hash;
        unsigned s = (unsigned)mix64(h) & K.map_mask;
        while (atomicCAS(&K.map[s], 0ull, map_entry(h, nw)) != 0ull) s = (s + 1) & K.map_mask;
    }
    if (blockIdx.x == 0 && tid == 0) {
        st->nparts = gridDim.x;
        if (!scan_only) {   // finish the trip: k rounds done; the state its select decided from
            st->round = B.round + k;
            st->ntok = B.ntok + (int)B.n_fresh;
            bs->trip = B.trip + 1;
            bs->prev_k = k;
            bs->prev_sparse = sparse;
            st->pool_used = B.pool_after;
            bs->batch_seq = B.batch_id;
            bs->T2 = b_T2;
            st->n_single += st->n_single_new;
            st->n_single_new = 0;
        }
    }
    if (pw0) probe_stamp(st, B.trip, 13);
    if (BPE355_PROBE_CODE && !scan_only && st->probe) {
        __syncthreads();
        if (tid == 0 && (B.trip % kProbeTrip) == 0) {   // workgroups that reserved list / C space
            unsigned long long* pr = st->probe + kProbeSlots * (size_t)(B.trip / kProbeTrip);
            if (s_nl) atomicAdd(&pr[22], 1ull);
            if (s_nc) atomicAdd(&pr[23], 1ull);
        }
        if (tid == 0) probe_done(st, &st->probe_apply_done, B.trip, 15);
    }
}

}  // namespace

}  // namespace bpe
