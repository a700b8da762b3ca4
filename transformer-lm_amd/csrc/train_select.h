// Merge loop, batched rounds: the batch rule, its constants and records, the probe helpers,
// select_core and k_select, the check kernels and k_snapshot.
// Part of train.hip, which includes the train_*.h headers in order into one translation unit
// (the helpers are file-local and the kernels inline them).
#pragma once
#include "train_round.h"

namespace bpe {

namespace {

// ------------------------------------------------------------------ batched rounds
// Several merges per round trip, exactly.  At a state S, let P1 > P2 > ... be the candidates in
// the reference's order (count, then bytes; train.py:187-189).  The top k form a batch when
//   (1) no member's b is any member's a (members may share an a, or share a b) and
//   (2) a != b for each (k > 1),
//   (3) each a + b is new bytes: not an existing token, not another member's (vocab.py:29),
//   (4) count(Pk) >= T and count(Pk) > count of the next candidate in C (keys outside C are
//       below T), so every pair outside the batch has a count strictly below count(Pk).
// Then the reference takes P1, ..., Pk in exactly that order:
//   * merging Pi = (ai, bi) removes only the pairs (x, ai) and (bi, y) at its occurrences; with
//     no b equal to an a, no member has either shape and no two members' occurrences overlap, so
//     Pj's count is unchanged until its turn; with a != b every occurrence of Pi is merged;
//   * an occurrence of a pair created by the batch sits where, before the batch, two original
//     tokens met -- an occurrence of an old pair that is not a member (members' occurrences are
//     all merged) -- so its count is below count(Pk); old non-members only lose counts.
// The rewrite applies the members in order to each word (the deltas of member j see the word
// after members < j, as the reference's sequence of rounds does), so counts, present keys and
// words after the trip equal the state after k rounds.
constexpr int kMaxBatch = 16;   // members per trip (3 * kMaxBatch tokens fit one wave)
static_assert(kMaxBatch >= 1 && kMaxBatch <= 21, "kMaxBatch: 1..21 (3 * members fit one wave)");
// the largest power of two <= kMaxBatch - 1: the first step of a binary search over members
constexpr int top_step(int m) { int p = 1; while (2 * p <= m) p *= 2; return m >= 1 ? p : 0; }
constexpr int kListTopStep = top_step(kMaxBatch - 1);
constexpr int kTopM = kMaxBatch + 1;
// the select's clash check: candidates i < kClashI (a power of two >= kMaxBatch), kClashJ lanes each
constexpr int kClashI = kMaxBatch <= 16 ? 16 : 32;
constexpr int kClashJ = 64 / kClashI;
constexpr unsigned kLdsB = 128;   // LDS-summed cells per member (ids below kLdsB)
// The least dense token prefix (CellMarks::dense_tok; the test knob BPE355_DENSE_TOK is clamped to
// it).  The merge marks touched blocks from cell 2 * dense_tok on, and the cells below 2 * kLdsB
// are flushed from LDS without setting touched-block bits: they must lie in the dense prefix,
// which every apply scans.
constexpr unsigned kDenseTokMin = 128;
static_assert(kLdsB <= kDenseTokMin, "LDS-summed cells are flushed unmarked: the dense prefix must cover them");
// Batch members may share an a or a b (rule (1)): with every member's tokens distinct from the
// others', that rule alone ended 2583 of 3682 batches on the bench corpus's merge sequence,
// against 498 of 2430 (tools/sim_batch.py, cap 16).  A tied non-member that seeds member j's new
// pairs cuts the batch after P_j (rule (4')), not back to the members above the tie.  (Both
// alternatives were build knobs of rounds 1-4: DESIGN.md section 4, "Batched merge rounds".)
// A word several members hit has all of them rewritten in registers, with one store pass, up to
// this slot width; the 64-id class (~60 more VGPRs) goes one member at a time through memory
constexpr int kRegRewriteMaxW = 32;
// Which members a word holds: with at least this many members, each adjacent pair of the word is
// looked up in an LDS table of the batch's pairs (hashed, 4096 one-byte slots: member + 1, 0xFF
// when two members share a slot) instead of compared with every member -- k x (W - 2) compares
// made the full scans of the first trips VALU-bound.
constexpr int kPairFilterK = 4;
static_assert(kPairFilterK >= 1, "members from which the pair table is used");
constexpr unsigned kPairSlots = 4096;
__device__ __forceinline__ unsigned pair_h12(unsigned x, unsigned y) {
    return ((x * 0x9E3779B1u) ^ (y * 0x85EBCA77u)) >> 20;
}
typedef __attribute__((address_space(3))) uint8_t LdsU8;

struct BatchMember {
    unsigned a, b, nw, slot;
    long long cnt;
    unsigned long long hash, k8, pw;
    unsigned ln, list_beg, list_len, use_list, cov_beg, cov_len, pool_off, isnew;
    // members sharing a token: the first member with this a (ga) / this b (gb) holds the mask of
    // every member with it, the others 0.  The apply updates (x, a) and (b, y) once, from the
    // group's summed cells (a key has one updater).
    unsigned ga, gb;
};
struct Batch {
    int stop;            // 0 run, -1 nothing to do, > 0 the halt the apply raises
    int k;               // members
    int round, ntok;     // round of member 0, token count before the batch
    int trip, prev_k;    // trip number (cell parity), members of the previous trip
    int prev_sparse;     // the previous trip's apply listed touched blocks (its merge clears by them)
    unsigned batch_id;   // word claims of this batch
    unsigned full_scan;  // a member has no usable posting list: scan every word once
    unsigned n_fresh;    // members that create a token
    unsigned nC_base;    // C entries before this trip's admissions (the apply scans them)
    unsigned idle_from;  // list mode: merge threads from this index on have no word (~0: scan mode)
    // state the select decided that its own kernel must not see change (every workgroup of the
    // fused trip kernel runs the select on the same inputs): the apply publishes them
    unsigned pool_after; // st->pool_used after this trip's new tokens
    long long T2next;    // the candidate-list threshold of this trip's apply (-> bs->T2)
    unsigned list_pre[kMaxBatch + 1];   // prefix sums of the members' list lengths
    BatchMember m[kMaxBatch];
};

// device-owned batch state (the host only initializes it; its limits live in RoundState)
struct BatchState {
    unsigned pend_insert;    // unused (k_apply_batch inserts the batch's new tokens into the map)
    unsigned batch_seq;      // last batch_id handed out
    int trip;                // trips completed
    int prev_k;              // members of the last trip (its cells are cleared by the next apply)
    int prev_sparse;         // the last trip's apply listed touched blocks (CellMarks)
    unsigned long long rounds_batched;   // statistics: rounds taken in batches of k > 1
    unsigned long long trips_batched;
    long long T2;            // candidate-list threshold (>= T): every present key >= T2 is listed
    // keys the apply appended to the list, by trip parity: trip t's select reads list (t & 1), its
    // apply fills list ((t + 1) & 1) (> kListCap: overflow)
    unsigned list_n[2];
    unsigned long long n_overflow, n_headmiss, n_short, k_hist[kMaxBatch + 1];   // diagnostics
    unsigned long long k1_why[6];   // single-merge trips: P1 a == b / P1 not fresh / no list / P2 fails / tie / end
    // what ended each batch: the cap / the ranked list ran out / candidate k failed the token or
    // freshness rules / the count gap or a tie at the boundary cut it / P1 not batchable
    unsigned long long end_why[5];
};
// the candidate list the select ranks, one thread per entry (a multiple of 64; a trip whose list
// overflows it takes P1 alone and raises T2).  128 took 56 more trips at the bench config for the
// same merge phase (255.6 ms, profiles/r05/g_bench_default.log; r04: zk_list_cap_ab.txt)
constexpr unsigned kListCap = 256;
static_assert(kListCap % 64 == 0 && kListCap >= 64, "whole waves of list threads");
// k_apply_batch workgroups (k_select reads one partial each)
constexpr unsigned kApplyGrid = 512;

struct SelKey {   // a listed candidate as k_select's ranking reads it
    long long cnt;
    unsigned long long ka, kb, ab;   // key8 of a and of b; b << 32 | a
};

struct TokMetaS {
    unsigned long long ha, pb, hb, pa;   // hash(a), P^len(b), hash(b), P^len(a)
    unsigned la, lb, za, zb, ba, bb;     // lengths; posting lists of a and b (len, begin)
};

// A member's cells: ids below N summed in LDS per workgroup (32-bit: a cell never exceeds the
// member's own count, count(P_j) <= count(P_1), so `narrow` = count(P_1) < 2^32 holds for the
// whole batch; otherwise every add goes to the global cells), the rest by global atomics.
typedef __attribute__((address_space(3))) unsigned LdsU32;   // an LDS word (explicit address space)
// Touched blocks (the apply visits only the cells that can hold a delta): a member's cells
// from `mark_from` on (2 x the densely scanned token prefix, >= 2 N) are grouped in blocks of 64
// cells (32 tokens); every global add there sets its block's bit in the workgroup's LDS bitmap
// (word = cell >> 11), which the flush ORs into one of kTBRep global replicas per trip parity
// (fewer same-address atomics); the apply ORs the replicas and lists the touched blocks.
constexpr unsigned kTBRep = 2;      // global bitmap replicas (a workgroup ORs into blockIdx % kTBRep)
constexpr unsigned kTBMax = 64;     // bitmap words per member: tokens up to 65 536 (else every cell scanned)
constexpr unsigned kTLCap = 4096;   // touched blocks the apply lists in LDS (more: every cell scanned)
struct CellMarks {
    unsigned* tb;        // [parity][kTBRep][kMaxBatch][tbw] touched-block bitmaps written by the merge
    unsigned* tbc;       // [kMaxBatch][tbw]: the last apply's OR of its replicas (the next merge clears by it)
    unsigned tbw;        // bitmap words per member (0: no marks, every cell scanned and cleared)
    unsigned dense_tok;  // tokens below this are scanned densely for every member (a multiple of 32)
    unsigned sparse_from;   // an apply lists touched blocks once the tokens pass this (below: every cell)
    unsigned long long* sig;   // BPE355_CHECK_MARKS: each apply workgroup's view of the list (else null)
};
template <unsigned N>
struct DeltaSinkN {
    unsigned long long* LR;     // this member's global cells
    LdsU32* lds;                // this member's LDS cells (ids below N)
    LdsU32* bm;                 // this member's touched-block bitmap (LDS)
    unsigned mark_from;         // cells from here on are marked (~0u: none)
    bool narrow;
    __device__ __forceinline__ void add(unsigned cell, unsigned long long c) const {
        if (narrow && cell < 2 * N) {
            __hip_atomic_fetch_add(&lds[cell], (unsigned)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            atomicAdd(&LR[cell], c);
            if (cell >= mark_from)
                __hip_atomic_fetch_or(&bm[cell >> 11], 1u << ((cell >> 6) & 31), __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
};

// BPE355_PROBE: 100 MHz stamps of one trip in kProbeTrip, kProbeSlots per sampled trip
// (MergeLoop::report_probe): 0-13 phase stamps, 14/15 the last merge/apply workgroup done, 16 the
// next trip's select start, 17-19 inside select's rule, 20/21 the last merge/apply workgroup's index
constexpr int kProbeTrip = 8;
constexpr int kProbeSlots = 32;   // 24-28: inside k_select's first phase
// The stamps are compiled in only with -DBPE355_PROBE_CODE=1 (tools/build_variant.sh probe; then
// the run-time BPE355_PROBE switch turns them on).  Compiled in but off, their code and registers
// cost 4-6 ms of the 260 ms merge phase (r04r A/B, two reps, profiles/r04/r_*).
#ifndef BPE355_PROBE_CODE
#define BPE355_PROBE_CODE 0
#endif
// The select's diagnostic counters (list overflows, head misses, the k histogram and why trips
// took one merge; printed under BPE355_TRACE) are compiled in only with -DBPE355_STATS_CODE=1.
// n_rounds_batched comes from the trips' records on the host either way.
#ifndef BPE355_STATS_CODE
#define BPE355_STATS_CODE 0
#endif
__device__ __forceinline__ void probe_stamp(const RoundState* st, int trip, int k) {
    if (BPE355_PROBE_CODE && st->probe && (trip % kProbeTrip) == 0)
        st->probe[kProbeSlots * (size_t)(trip / kProbeTrip) + k] = __builtin_amdgcn_s_memrealtime();
}
// one workgroup of a sampled trip's kernel is done (thread 0, after the workgroup's work): the
// last of the grid stamps slot k
__device__ __forceinline__ void probe_done(RoundState* st, unsigned* ctr, int trip, int k) {
    if (BPE355_PROBE_CODE && st->probe && (trip % kProbeTrip) == 0) {
        const unsigned o = atomicAdd(ctr, 1u);
        if (o % gridDim.x == gridDim.x - 1) {
            probe_stamp(st, trip, k);
            st->probe[kProbeSlots * (size_t)(trip / kProbeTrip) + k + 6] = blockIdx.x + 1;
        }
    }
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int j) {
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, j);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}
// lane j's candidate, in every lane (scalar broadcast)
__device__ __forceinline__ Cand readlane_cand(const Cand& c, int j) {
    Cand r;
    r.cnt = (long long)readlane64((unsigned long long)c.cnt, j);
    r.ka = readlane64(c.ka, j);
    r.kb = readlane64(c.kb, j);
    r.slot = __builtin_amdgcn_readlane((int)c.slot, j);
    r.a = __builtin_amdgcn_readlane((int)c.a, j);
    r.b = __builtin_amdgcn_readlane((int)c.b, j);
    return r;
}

// The wave's best candidate in every lane.  The order is the count first (cand_better), so the
// wave's largest count is found with 64-bit shuffles alone; its holder's candidate is the best
// when it is the only one (then read from that lane), and only a tie at the top goes through the
// full order (shuffles of the whole candidate, and the bytes when the 8-byte prefixes tie).
__device__ __forceinline__ Cand wave_best(Cand best, const ToksDev& K) {
    {   // the count-only shortcut (scoped: k_select's register allocation depends on m and hold ending here)
        long long m = best.cnt;
        for (int o = 32; o > 0; o >>= 1) m = max(m, (long long)__shfl_xor(m, o));
        if (m == LLONG_MIN) return cand_none();
        const unsigned long long hold = __ballot(best.cnt == m);
        if (__popcll(hold) == 1) return readlane_cand(best, __ffsll((long long)hold) - 1);
        if (best.cnt != m) best = cand_none();
    }
    for (int o = 32; o > 0; o >>= 1) {
        const Cand oc = shfl_xor_cand(best, o);
        if (cand_better(oc, best, K.pool, K.off, K.len)) best = oc;
    }
    return best;
}

// A listed candidate's token metadata and dedupe lookup (does the pair's byte string exist as a
// token already?).  The map holds every token up to the last trip's (k_apply_batch inserts them).
__device__ __forceinline__ void cand_meta(const Cand& c, const ToksDev& K, const IndexDev& X, TokMetaS& m,
                                          unsigned& old) {
    const unsigned a = c.a, b = c.b;
    m.ha = K.hash[a]; m.pb = K.pw[b]; m.hb = K.hash[b]; m.pa = K.pw[a];
    m.la = K.len[a]; m.lb = K.len[b];
    m.za = X.len[a]; m.zb = X.len[b]; m.ba = X.beg[a]; m.bb = X.beg[b];
    const unsigned long long h = m.ha * m.pb + m.hb;
    const unsigned ln = m.la + m.lb;
    old = map_find(K, h, ln, a, b);
}

// One workgroup: the batch of this trip.  Waves 0-7 reduce the apply's per-workgroup partials
// to the exact best candidate P1; waves 8-11 hold the candidate list (every present key >= T2),
// look up its entries' metadata and rank them.  All global loads are issued before the first
// barrier, so the kernel costs about one memory round trip plus the dedupe lookups' chain, then
// the ranking, the rule and the record (wave 0).
constexpr unsigned kListTarget = 48;   // keys the next list should hold (T2 control)
// waves of k_select that reduce the apply's partials (kPartPer each per thread); the list's waves
// follow them.  4 waves with two partials per thread: a 512-thread select, 252.2-253.7 ms of
// HBM-resident merges against 255.0-268.0 with 8 waves and 258.3-260.6 with 2 (two paired reps,
// profiles/r04/zh_*)
constexpr int kSelListWave = 4;   // first wave of the list
constexpr bool kSelMetaAll = true;     // metadata of every listed key before the ranking
constexpr int kSelThreads = 64 * kSelListWave + (int)kListCap;
// k_trip workgroups: 256 threads (four per CU).  One 1024-thread workgroup per CU decided faster
// (the partials' re-reads by four workgroups per CU cost 1.3 us) but left an 11.8 us merge ->
// apply gap: 289 vs 258 ms of merges (profiles/r05/d_fold_ab.txt)
constexpr unsigned kTripThreads = 256;

// The LDS of one batch decision
struct SelLds {
    Cand wave[8];                     // the partial waves' bests
    Cand all[kListCap];
    SelKey topkey[kListCap];          // the entries with fewer than kTopM larger counts,
    unsigned top[kListCap];           // packed for the exact ranking (key, list index)
    long long cnt[kListCap];
    Cand list[kTopM];
    TokMetaS meta[kTopM];
    unsigned nw_old[kTopM];
    Cand p1;                          // the exact best (wave 0, beside the ranking)
    long long cnt_target, cnt_last;   // counts at sorted positions kListTarget - 1, ln - 1
    unsigned ntop;
};

// where the publishing workgroup records a batch decision for the host (round records, the
// block's trip records)
constexpr int kTI = 8;   // ints per trip record: round, k, full scan, list entries, ntok, |C|, listed keys, fresh
struct SelOut {
    uint32_t *m_a, *m_b, *m_new, *m_mode;
    long long* m_cnt;
    int* trip_info;
    int trip_slot;
};

// The batch of a trip: reduce the apply's per-workgroup partials to the exact best candidate P1,
// rank the candidate list (every present key >= T2) and apply the batch rule.  All global loads
// are issued first, so the decision costs about one memory round trip plus the dedupe lookups'
// chain, then the ranking, the rule and the record (wave 0).
//   kNT = kSelThreads (k_select, one workgroup): waves 0-3 reduce the partials while the list
//         waves rank;
//   kNT = 256 (k_trip: EVERY workgroup of the fused trip kernel decides the same batch): each
//         thread reduces two partials and holds one list entry.
// The decision goes to OB (stop != 0: no trip this time; > 0 a halt code the apply raises).
// It reads only state that no kernel of the trip changes before the apply: the select phase of
// k_trip runs in every workgroup while other workgroups already rewrite, so everything it decides
// from (st->n_single, pool_used, halt, the list counts, batch_seq, T2) is updated by the apply,
// from the batch record.  `pub`: this workgroup publishes (the round records, trip records, the
// next list's counter, the statistics).  The caller's barrier makes OB visible.
template <int kNT>
__device__ __forceinline__ void select_core(const RoundState* __restrict__ st, BatchState* __restrict__ bs,
                                            const ToksDev& K, const IndexDev& X,
                                            const Partial* __restrict__ part, const Partial* __restrict__ lists,
                                            Batch& OB, SelLds& S, const SelOut& O, const bool pub) {
    static_assert(kNT == kSelThreads || kNT == 256 || kNT == 1024,
                  "k_select's shape, or one k_trip workgroup of 256 or 1024 threads");
    // threads that reduce partials (the first kPartT) and the list thread of each entry (a
    // 1024-thread k_trip workgroup decides as k_select does; its other waves wait at the barriers)
    constexpr int kPartT = kNT == 256 ? kNT : 64 * kSelListWave;
    constexpr int kPartW = kPartT / 64;
    constexpr int kListT0 = kNT == 256 ? 0 : 64 * kSelListWave;
    static_assert(kPartW <= 8 && (int)kListCap <= kNT - kListT0, "one list entry per list thread");
    constexpr int kPartPer = (int)((kApplyGrid + kPartT - 1) / kPartT);
    static_assert(kPartPer >= 1 && kPartPer <= 4, "partials per thread of the partial waves");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ptrip = bs->trip;
    if (pub && tid == 0) {
        probe_stamp(st, ptrip, 0);
        if (BPE355_PROBE_CODE && ptrip > 0 && st->probe && ((ptrip - 1) % kProbeTrip) == 0)
            st->probe[kProbeSlots * (size_t)((ptrip - 1) / kProbeTrip) + 16] = __builtin_amdgcn_s_memrealtime();
    }
    // ---- every independent load first
    Partial q[kPartPer] = {};
    if (tid < kPartT) {   // the buffer holds kApplyGrid entries
#pragma unroll
        for (int u = 0; u < kPartPer; ++u)
            if (tid + u * kPartT < (int)kApplyGrid) q[u] = part[tid + u * kPartT];
    }
    const Partial* list = lists + (size_t)(ptrip & 1) * kListCap;   // this trip's list (trip parity)
    Partial lq{};
    // list entry of this thread (>= 0: list threads)
    const int li = tid >= kListT0 && tid < kListT0 + (int)kListCap ? tid - kListT0 : -1;
    if (li >= 0) lq = list[li];
    const int nparts = st->nparts;
    const unsigned ln = bs->list_n[ptrip & 1];
    if (st->halt) {   // a trip queued behind a halt: nothing to do (the host takes over)
        if (tid == 0) {
            OB.stop = -1;
            if (pub && O.trip_info) {
                int* ti = O.trip_info + kTI * O.trip_slot;
                ti[0] = -1; ti[1] = 0; ti[2] = 0; ti[3] = 0;
            }
        }
        return;
    }
    // the rule's scalars (uniform: scalar loads, in flight with the vector loads above)
    const int round = st->round, n_rounds = st->n_rounds, host_round = st->host_round;
    const unsigned nC = st->nC, c_limit = st->c_limit;
    const long long T = st->T;
    const unsigned n_single = st->n_single, single_limit = st->single_limit;
    const unsigned long long pair_used = st->pair_used, pair_limit = st->pair_limit;
    const unsigned pool_used = st->pool_used, pool_cap = st->pool_cap;
    const unsigned max_len = st->max_len;
    const int ntok = st->ntok, max_batch = st->max_batch;
    const int prev_k = bs->prev_k, prev_sparse = bs->prev_sparse;
    const unsigned bid = bs->batch_seq + 1;
    const long long T2old = bs->T2;
    if (pub && tid == 0) probe_stamp(st, ptrip, 1);
    // the list: each entry's metadata first (its chain of dependent loads overlaps the partials'
    // arrival), then each entry's rank among the entries
    const int nl = ln <= kListCap ? (int)ln : 0;
    const bool have = li >= 0 && li < nl;
    const Cand x = have ? Cand{lq.cnt, lq.ka, lq.kb, lq.slot, lq.a, lq.b} : cand_none();
    TokMetaS lm{};
    unsigned lold = ~0u;
    if (li >= 0) {
        if (li < kTopM) S.list[li] = cand_none();
        if (li == 0) { S.cnt_target = LLONG_MAX; S.cnt_last = LLONG_MAX; S.ntop = 0; }
        S.all[li] = x;
        S.cnt[li] = x.cnt;
        if (pub && li == 0 && lq.slot != 0xfffffffeu) probe_stamp(st, ptrip, 24);   // the list entry arrived
        if (have && kSelMetaAll) cand_meta(x, K, X, lm, lold);
        if (pub && li == 0 && lold != 0xfffffffeu && lm.la != 0xfffffffeu) probe_stamp(st, ptrip, 25);   // metadata + dedupe
    }
    if (tid < kPartT) {   // P1: the exact best over the partials
        Cand best = cand_none();
#pragma unroll
        for (int u = 0; u < kPartPer; ++u) {
            const int idx = tid + u * kPartT;
            if (idx < nparts) {
                const Cand c{q[u].cnt, q[u].ka, q[u].kb, q[u].slot, q[u].a, q[u].b};
                if (cand_better(c, best, K.pool, K.off, K.len)) best = c;
            }
        }
        best = wave_best(best, K);
        if (lane == 0) S.wave[wv] = best;
    }
    if (pub && tid == 0) probe_stamp(st, ptrip, 26);   // wave 0's partials reduced
    if (BPE355_PROBE_CODE && pub && tid == 0 && st->probe && (ptrip % kProbeTrip) == 0)
        st->probe[kProbeSlots * (size_t)(ptrip / kProbeTrip) + 30] = ln + 1;
    __syncthreads();
    if (pub && li == 0) probe_stamp(st, ptrip, 27);
    if (wv == 0) {   // P1 over the waves' bests, while the list waves rank (off the rule's path)
        Cand p = S.wave[0];
        for (int w = 1; w < kPartW; ++w)
            if (cand_better(S.wave[w], p, K.pool, K.off, K.len)) p = S.wave[w];
        if (lane == 0) S.p1 = p;
    }
    long long tgt = LLONG_MAX, last = LLONG_MAX;
    // rank by count alone first (one 8-byte compare per entry); only an entry with fewer than
    // kTopM larger counts can be among the first kTopM, and every entry ordered before such an
    // entry has its count or a larger one, so it has fewer than kTopM larger counts too: the
    // exact order among that small set is the exact order overall
    int rc = kTopM, ec = 0;   // entries with a larger count, with an equal count (itself included)
    if (have) {
        rc = 0;
#pragma unroll 8
        for (int j = 0; j < nl; ++j) {
            const long long cj = S.cnt[j];
            rc += cj > x.cnt ? 1 : 0;
            ec += cj == x.cnt ? 1 : 0;
        }
        if (rc < kTopM) {
            const unsigned pos = atomicAdd(&S.ntop, 1u);
            S.top[pos] = li;
            S.topkey[pos] = SelKey{x.cnt, x.ka, x.kb, (unsigned long long)x.b << 32 | x.a};
        }
        // the count at sorted position t is the least count whose first position is <= t
        tgt = rc <= (int)kListTarget - 1 ? x.cnt : LLONG_MAX;
        last = x.cnt;
    }
    if (pub && li == 0) probe_stamp(st, ptrip, 29);   // count ranks done
    __syncthreads();
    if (pub && li == 0) probe_stamp(st, ptrip, 31);   // every list thread's count rank done
    if (have && rc < kTopM) {
        // (count, a's 8-byte prefix, b's) branch-free over the small set; only equal prefixes of
        // different tokens need the bytes (rare: then cand_better).  With no other entry of its
        // count, the count rank is the exact rank (the usual case); otherwise the ties are ordered
        // by bytes over the packed top entries, which hold every entry of this count (each has
        // the same rc < kTopM)
        const int m = ec > 1 ? (int)S.ntop : 0;
        int rank = ec > 1 ? 0 : rc;
        bool tail = false;
#pragma unroll 4
        for (int t = 0; t < m; ++t) {
            const int j = (int)S.top[t];
            const SelKey y = S.topkey[t];
            const unsigned ya = (unsigned)y.ab, yb = (unsigned)(y.ab >> 32);
            const bool gt = y.cnt > x.cnt, eq = y.cnt == x.cnt && j != li;
            const bool ad = ya != x.a, bd = yb != x.b;
            rank += gt | (eq & ad & (y.ka > x.ka)) | (eq & !ad & bd & (y.kb > x.kb));
            tail |= eq & ((ad & (y.ka == x.ka)) | (!ad & bd & (y.kb == x.kb)));
        }
        if (tail) {
            rank = 0;
            for (int t = 0; t < m; ++t) {
                const int j = (int)S.top[t];
                rank += (j != li && cand_better(S.all[j], x, K.pool, K.off, K.len)) ? 1 : 0;
            }
        }
        if (rank < kTopM) {
            if (!kSelMetaAll) cand_meta(x, K, X, lm, lold);
            S.list[rank] = x;
            S.meta[rank] = lm;
            S.nw_old[rank] = lold;
        }
    }
    if (pub && li == 0) probe_stamp(st, ptrip, 28);   // ranked
    if (li >= 0 && (kListT0 > 0 || wv < (int)(kListCap / 64))) {   // wave minima, then one LDS atomic per wave
        for (int o = 32; o > 0; o >>= 1) {
            tgt = min(tgt, (long long)__shfl_xor(tgt, o));
            last = min(last, (long long)__shfl_xor(last, o));
        }
        if (lane == 0 && last != LLONG_MAX) {
            atomicMin(&S.cnt_target, tgt);
            atomicMin(&S.cnt_last, last);
        }
    }
    __syncthreads();
    if (pub && tid == 0) probe_stamp(st, ptrip, 2);
    if (wv != 0) return;
    // ---- wave 0: the rule and the record, lane i holding candidate i (no workgroup barrier)
    const Cand p1 = S.p1;
    // the list's head is the global best whenever the best is >= T2 and nothing overflowed; the
    // ranks are distinct, so S.list holds a prefix
    if (pub && lane == 0) probe_stamp(st, ptrip, 17);
    const bool list_ok = ln <= kListCap && S.list[0].cnt != LLONG_MIN && S.list[0].slot == p1.slot &&
                         S.list[0].a == p1.a && S.list[0].b == p1.b;
    int nf = 1;
    if (list_ok) {
        const unsigned long long vm =
            __ballot(lane >= 1 && lane < kTopM && S.list[lane < kTopM ? lane : 0].cnt != LLONG_MIN) | 1ull;
        nf = __builtin_ctzll(~vm);
    }
    int stop = HALT_NONE;
    if (round >= n_rounds) stop = HALT_DONE;
    else if (nC > c_limit) stop = HALT_REBUILD;                        // C bloated: re-threshold
    else if (p1.cnt == LLONG_MIN || p1.cnt < T) stop = HALT_REBUILD;   // max(C) < T: re-threshold
    else if (round >= host_round || n_single > single_limit ||
             pair_used + 2ull * (unsigned)(ntok + kMaxBatch) * kMaxBatch > pair_limit ||
             pool_used + (unsigned long long)kMaxBatch * max_len > pool_cap)
        stop = HALT_HOST;
    if (BPE355_STATS_CODE && pub && lane == 0) {   // no-return atomics: nothing waits on them
        if (ln > kListCap) atomicAdd(&bs->n_overflow, 1ull);
        else if (!list_ok) atomicAdd(&bs->n_headmiss, 1ull);
        else if (nf < kTopM) atomicAdd(&bs->n_short, 1ull);
    }
    if (stop) {   // the apply raises the halt (nothing this trip's kernels read changes before it)
        if (lane == 0) {
            OB.stop = stop;
            if (pub && O.trip_info) {
                int* ti = O.trip_info + kTI * O.trip_slot;
                ti[0] = -1; ti[1] = 0; ti[2] = 0; ti[3] = 0;
            }
        }
        return;
    }
    const int i = lane;
    Cand e = cand_none();
    TokMetaS m{};
    unsigned old = ~0u;
    if (i == 0) {
        e = p1;
        if (list_ok) { m = S.meta[0]; old = S.nw_old[0]; }
        else cand_meta(p1, K, X, m, old);   // rare: P1 alone, its metadata here
    } else if (i < nf) {
        e = S.list[i];
        m = S.meta[i];
        old = S.nw_old[i];
    }
    const bool fr = i < nf && old == ~0u;
    if (pub && lane == 0) probe_stamp(st, ptrip, 18);
    const unsigned long long h = m.ha * m.pb + m.hb;
    const unsigned lk = m.la + m.lb;
    // (1) a different from every earlier candidate's b and b from every earlier a, and (3) new
    // bytes different from every earlier candidate's.
    // The kClashI x kClashI (i, j) pairs are spread over the wave: lane L checks i = L % kClashI
    // against j = L / kClashI + t * kClashJ, then the kClashJ lanes of each i combine (one pass of
    // lane shuffles instead of a serial readlane chain over j)
    // each candidate's posting list (the shorter of a's and b's) and whether the merge uses it
    const unsigned lu = m.za <= m.zb ? m.za : m.zb, bu = m.za <= m.zb ? m.ba : m.bb;
    const bool use = lu != kNoAnc && lu <= X.full_threshold;
    const unsigned long long lkey = use && lu > 0 ? (unsigned long long)bu << 32 | lu : 0ull;
    bool clash = false;
    // beside the clash check, for the members' token groups: the candidates with i's
    // a (sa) and with i's b (sb), and whether an earlier candidate walks i's posting list (dl)
    unsigned sa = 0, sb = 0;
    bool dl = false;
    {
        const int ci = lane % kClashI, cj0 = lane / kClashI;
        const unsigned ai = __shfl((int)e.a, ci), bi = __shfl((int)e.b, ci);
        const unsigned long long hi = __shfl(h, ci);
        const unsigned li_ = __shfl((int)lk, ci), lai = __shfl((int)m.la, ci);
        const unsigned long long lki = __shfl(lkey, ci);
        const bool iv = ci < nf;
#pragma unroll
        for (int t = 0; t < (kTopM + kClashJ - 1) / kClashJ && t < kClashI / kClashJ; ++t) {
            const int j = cj0 + t * kClashJ;   // (candidates past kTopM - 1 are never ranked)
            const unsigned aj = __shfl((int)e.a, j), bj = __shfl((int)e.b, j);
            const unsigned long long hj = __shfl(h, j);
            const unsigned lj = __shfl((int)lk, j), laj = __shfl((int)m.la, j);
            const unsigned long long lkj = __shfl(lkey, j);
            sa |= (unsigned)(aj == ai) << j;
            sb |= (unsigned)(bj == bi) << j;
            dl |= j < ci && lki != 0 && lkj == lki;
            if (j < ci && iv) {
                const bool tc = aj == bi || bj == ai;
                clash |= tc;
                if (!tc && hj == hi && lj == li_) {   // equal hashes: compare the bytes (rare)
                    bool eq = true;
                    for (unsigned y = 0; y < li_ && eq; ++y)
                        eq = concat_byte(K, aj, laj, bj, y) == concat_byte(K, ai, lai, bi, y);
                    clash |= eq;
                }
            }
        }
        for (int o = kClashI; o < 64; o <<= 1) {
            clash |= __shfl_xor((int)clash, o) != 0;
            sa |= (unsigned)__shfl_xor((int)sa, o);
            sb |= (unsigned)__shfl_xor((int)sb, o);
            dl |= __shfl_xor((int)dl, o) != 0;
        }
        if (i >= kClashI) clash = false;   // lanes < kClashI hold their own i's result
    }
    // k: the first candidate that fails (count >= T, (2) a != b, fresh, no clash), within the
    // allowed batch; one merge when P1 itself is not batchable
    const int maxb = min(max_batch, kMaxBatch);
    const bool okb = i >= 1 && i < nf && e.cnt >= T && e.a != e.b && fr && !clash;
    int k = __builtin_ctzll(~(__ballot(okb) | 1ull));
    k = min(k, min(maxb, nf));
    const int k_rule = k;
    if (!(p1.a != p1.b && __builtin_amdgcn_readlane((int)fr, 0))) k = 1;
    // (4) strictly above the next candidate: listed (candidate k), or unlisted (below T2, and
    // every member is listed, so >= T2): the largest k' <= k with that gap
    {
        const long long cprev = __shfl(e.cnt, i > 0 ? i - 1 : 0);
        const unsigned long long gm =
            __ballot(i >= 1 && (i >= nf || cprev > e.cnt)) & ((2ull << k) - 1) & ~1ull;
        const int k_strict = gm ? 63 - __builtin_clzll(gm) : 1;
        // (4') a tie at the boundary is harmless unless a tied non-member could seed a new pair:
        // a pair created by the batch has at most the count of the old pair (x, a_j) or (b_j, y)
        // it replaces, so with every tied non-member free of those shapes, no new pair reaches
        // count(Pk).  Every key >= T2 is listed, so the tied keys are all in S.all.  A pair
        // member j creates exists only after P_j's merge, so it can precede only members after j:
        // with j the first member a tied non-member seeds, the batch keeps P1 .. P_j (and at
        // least the members above the tie).  Former members past the cut never seed one (no b
        // of one member is another's a), so the shorter batch needs no second check.
        if (k_strict < k && k > 1) {
            const long long c = readlane64((unsigned long long)e.cnt, k - 1);
            unsigned ma[kMaxBatch], mb[kMaxBatch], ms[kMaxBatch];
#pragma unroll
            for (int j = 0; j < kMaxBatch; ++j) {
                ma[j] = __builtin_amdgcn_readlane((int)e.a, j);
                mb[j] = __builtin_amdgcn_readlane((int)e.b, j);
                ms[j] = __builtin_amdgcn_readlane((int)e.slot, j);
            }
            int jb = k;   // the first member a tied non-member seeds (k: none)
            for (int t = lane; t < nl; t += 64) {
                const Cand y = S.all[t];
                if (y.cnt != c) continue;
                bool member = false;
                int js = k;
#pragma unroll
                for (int j = 0; j < kMaxBatch; ++j) {
                    if (j >= k) break;
                    member |= y.slot == ms[j];
                    if (js == k && (y.b == ma[j] || y.a == mb[j])) js = j;
                }
                if (!member) jb = min(jb, js);
            }
            for (int o = 32; o > 0; o >>= 1) jb = min(jb, __shfl_xor(jb, o));
            k = min(k, max(jb + 1, k_strict));
        } else {
            k = k_strict;
        }
    }
    if (pub && lane == 0) probe_stamp(st, ptrip, 19);
    const bool fr0 = __builtin_amdgcn_readlane((int)fr, 0);
    if (BPE355_STATS_CODE && pub && k == 1 && lane == 0) {
        const int why = p1.a == p1.b ? 0 : !fr0 ? 1 : nf == 1 ? 2 : k_rule == 1 ? 3 : 4;
        atomicAdd(&bs->k1_why[why], 1ull);
    }
    if (BPE355_STATS_CODE && pub && lane == 0) {
        const int why = !(p1.a != p1.b && fr0) ? 4 : k < k_rule ? 3 : k_rule == maxb ? 0 : k_rule == nf ? 1 : 2;
        atomicAdd(&bs->end_why[why], 1ull);
    }
    k = min(k, n_rounds - round);
    // per member: pool offset, new id, posting-list prefix (exclusive scans over lanes < k)
    const bool mem = i < k;
    // the members' token groups (equal a's, equal b's: the group's first member carries the
    // group's mask) and posting lists two members share (the later one walks none of it: the
    // word is claimed once and every member's hits are found on it)
    const unsigned km = (unsigned)((1ull << k) - 1), below = (1u << (i & 31)) - 1;
    unsigned ga = sa & km, gb = sb & km;
    if (ga & below) ga = 0;
    if (gb & below) gb = 0;
    const bool dup_list = dl;   // (an earlier candidate with the list is a member when i is)
    const unsigned add_pool = mem && fr ? lk : 0u, add_fresh = mem && fr ? 1u : 0u,
                   add_list = mem && use && !dup_list ? lu : 0u;
    unsigned pre_pool = add_pool, pre_fresh = add_fresh, pre_list = add_list;   // inclusive scans
    for (int d = 1; d <= kMaxBatch; d <<= 1) {
        const unsigned tp = __shfl_up((int)pre_pool, d), tf = __shfl_up((int)pre_fresh, d),
                       tl = __shfl_up((int)pre_list, d);
        if (lane >= d) { pre_pool += tp; pre_fresh += tf; pre_list += tl; }
    }
    pre_pool -= add_pool; pre_fresh -= add_fresh; pre_list -= add_list;   // exclusive: lanes < i
    // one scan of every word once the members' lists together pass the scan threshold
    const bool full = __ballot(mem && !use) != 0 || __builtin_amdgcn_readlane((int)pre_list, k) > (int)X.full_threshold;
    const unsigned tot_pool = __builtin_amdgcn_readlane((int)pre_pool, k);
    const unsigned tot_list = __builtin_amdgcn_readlane((int)pre_list, k);
    const unsigned tot_fresh = __builtin_amdgcn_readlane((int)pre_fresh, k);
    if (i <= k) OB.list_pre[i] = pre_list;
    if (mem) {
        BatchMember M;
        M.a = e.a; M.b = e.b; M.slot = e.slot; M.cnt = e.cnt;
        M.nw = fr ? (unsigned)ntok + pre_fresh : old;
        M.isnew = fr;
        M.hash = h;
        M.pw = m.pa * m.pb;
        M.ln = lk;
        M.k8 = m.la >= 8 ? e.ka : (e.ka | (e.kb >> (8 * m.la)));
        M.use_list = use;
        M.list_beg = use ? bu : 0;
        M.list_len = use ? lu : 0;
        M.cov_beg = bu;
        M.cov_len = fr ? lu : kNoAnc;   // dedupe: uncovered until the next index build
        M.pool_off = pool_used + pre_pool;
        M.ga = ga;
        M.gb = gb;
        OB.m[i] = M;
        if (pub) {
            O.m_a[round + i] = e.a; O.m_b[round + i] = e.b; O.m_new[round + i] = M.nw;
            O.m_mode[round + i] = use ? lu : 0xffffffffu;
            if (O.m_cnt) O.m_cnt[round + i] = e.cnt;
        }
    }
    if (lane == 0) {
        OB.stop = 0;
        OB.k = k;
        OB.round = round;
        OB.ntok = ntok;
        OB.trip = ptrip;
        OB.prev_k = prev_k;
        OB.prev_sparse = prev_sparse;
        OB.batch_id = bid;
        OB.nC_base = nC;
        OB.full_scan = full;
        {   // the merge's idle workgroups: past the listed words, when every member has a list
            const bool lists_ok = k > 1 ? !full : use;   // lane 0: member 0's own flag
            OB.idle_from = lists_ok ? tot_list : ~0u;
        }
        OB.n_fresh = tot_fresh;
        OB.pool_after = pool_used + tot_pool;
        {   // the next list: about kListTarget keys.  With the list ranked, T2 = the count of the
            // kListTarget-th best (this trip pops at most kMaxBatch of those above it); on overflow
            // raise T2 halfway to the top; with too few keys, extend the range below the last one
            const long long top = p1.cnt;
            const long long t2 = T2old < T ? T : T2old;
            long long nt;
            if (ln > kListCap) nt = t2 + (top - t2) / 2;
            else if (ln >= kListTarget) nt = S.cnt_target;
            else if (ln > 0) nt = S.cnt_last - (top - S.cnt_last) - 1;
            else nt = T;
            OB.T2next = nt < T ? T : (nt > top ? top : nt);
        }
        if (pub) {
            bs->list_n[(ptrip + 1) & 1] = 0;   // the list this trip's apply fills (nothing reads it before)
            if (BPE355_STATS_CODE) {
                if (k > 1) {
                    atomicAdd(&bs->rounds_batched, (unsigned long long)k);
                    atomicAdd(&bs->trips_batched, 1ull);
                }
                atomicAdd(&bs->k_hist[k], 1ull);
            }
            if (O.trip_info) {   // for the host: first round, members, scan mode, list entries
                int* ti = O.trip_info + kTI * O.trip_slot;
                ti[0] = round; ti[1] = k; ti[2] = full; ti[3] = (int)tot_list;
                // (the trip log's extra fields: tokens, C entries the apply scans, listed keys, fresh tokens)
                ti[4] = ntok; ti[5] = (int)nC; ti[6] = (int)ln; ti[7] = (int)tot_fresh;
            }
            probe_stamp(st, ptrip, 3);
            probe_stamp(st, ptrip, 4);
        }
    }
}

__global__ void __launch_bounds__(kSelThreads) k_select(const RoundState* __restrict__ st, BatchState* __restrict__ bs,
                                                        ToksDev K, IndexDev X, Batch* __restrict__ bt,
                                                        const Partial* __restrict__ part,
                                                        const Partial* __restrict__ lists, SelOut O) {
    __shared__ SelLds S;
    select_core<kSelThreads>(st, bs, K, X, part, lists, *bt, S, O, true);
}

// Test knob BPE355_CHECK_MARKS: after a trip's merge, the other parity (cleared by it from the
// dense prefix and the previous apply's touched-block list) must be zero in every cell and bitmap:
// a nonzero cell there is a delta the marks missed.  dbg[0] counts them, dbg[1..3] the first one
// (trip, member, cell).
__global__ void k_check_clear(const Batch* __restrict__ bt, const unsigned long long* __restrict__ LRbase,
                              size_t lr_member, size_t lr_parity, const unsigned* __restrict__ tb, unsigned tbw,
                              unsigned long long* __restrict__ dbg) {
    const Batch& B = *bt;
    if (B.stop) return;
    const unsigned long long* LRo = LRbase + (size_t)((B.trip + 1) & 1) * lr_parity;
    const size_t n = (size_t)kMaxBatch * lr_member;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x)
        if (LRo[q] != 0 && atomicAdd(&dbg[0], 1ull) == 0) {
            dbg[1] = (unsigned long long)B.trip;
            dbg[2] = q / lr_member;
            dbg[3] = q % lr_member;
        }
    if (tbw) {
        const unsigned* TBo = tb + (size_t)((B.trip + 1) & 1) * kTBRep * kMaxBatch * tbw;
        for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < (size_t)kTBRep * kMaxBatch * tbw;
             q += (size_t)gridDim.x * blockDim.x)
            if (TBo[q]) atomicAdd(&dbg[4], 1ull);
    }
}

// BPE355_CHECK_MARKS after an apply: every workgroup must have seen the same touched blocks
__global__ void k_check_sig(const Batch* __restrict__ bt, unsigned long long* __restrict__ sig, unsigned n,
                            unsigned long long* __restrict__ dbg) {
    const Batch& B = *bt;
    for (unsigned i = threadIdx.x; i < n; i += blockDim.x) {
        if (!B.stop && sig[1 + i] != sig[1] && atomicAdd(&dbg[5], 1ull) == 0) {
            dbg[6] = (unsigned long long)B.trip;
            dbg[7] = i;
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < n; i += blockDim.x) sig[1 + i] = 0;
}

// end of a block of trips: the state and the trips' records -> pinned host memory (plain vector
// stores; the block's event orders them before the host reads)
__global__ void __launch_bounds__(256) k_snapshot(const uint32_t* __restrict__ st, unsigned n_st,
                                                  const uint32_t* __restrict__ ti, unsigned n_ti,
                                                  uint32_t* __restrict__ h_st, uint32_t* __restrict__ h_ti) {
    for (unsigned i = threadIdx.x; i < n_st; i += blockDim.x) h_st[i] = st[i];
    for (unsigned i = threadIdx.x; i < n_ti; i += blockDim.x) h_ti[i] = ti[i];
}

}  // namespace

}  // namespace bpe
