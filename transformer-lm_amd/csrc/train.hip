// BPE merge loop on the device.
//
// Reference semantics (models/tokenizer/train.py):
//   31-49    words -> byte ids, pair histogram weighted by word count
//   183-189  rounds = vocab_size - len(vocab); best = max(pairs, key=(count, (bytes a, bytes b)))
//            over every key still in the dict (count 0 included); stop early only if empty
//   190-224  new = a + b; rewrite every word left to right, non-overlapping; per occurrence
//            (x, a) -= c, (x, new) += c for the rewritten left neighbour x, and
//            (b, y) -= c, (new, y) += c for the original right neighbour y
//   226-228  pop best; append (a, b) to merges
// Tokens are identified by their bytes (vocab.py:29): a merge whose bytes already exist
// reuses that token's id (token dedupe below).
//
// HBM layout of the unique-word table (the stream every round reads):
//   words live in fixed-width SLOTS of W token ids, W in {8, 16, 32, 64}: slot[0] = current
//   length, slot[1..] = ids, the unused tail filled with a sentinel id that never matches a
//   pair.  A 16-byte slot (u16 ids) is one dwordx4 load per word, coalesced across the wave,
//   and the pair test is W-2 register compares with no branch on the length.  Words longer
//   than 63 ids sit in a CSR side table.  Counts (u64) are a parallel array read only on a hit.
//   Words that shrink to one id drop out, and words migrate to narrower slots, at compaction.
//
// Per round, three kernels on one HIP stream (host checks state once per batch of rounds):
//   K1 k_merge  : every workgroup reduces K3's per-block partials to the round's best pair and
//                 resolves the new token id (hash map over token bytes); block 0 records the merge.
//                 Then all workgroups rewrite the words containing (a, b) and accumulate, per
//                 neighbour token, the deltas L[x] (left) and R[y] (right) as int64.
//   [one all-reduce of L/R over ranks when the corpus is sharded]
//   K2 k_apply  : 4 threads per token: (x,a)-=L[x], (x,new)+=L[x], (b,y)-=R[y], (new,y)+=R[y]
//                 on the pair hash table; touched keys become present; increments that lift a
//                 key across the threshold T append it to the candidate list C.
//   K3 k_argmax : argmax over C of (count, bytes a, bytes b) -> per-block partials; bytes
//                 compare by 8-byte big-endian prefix, the pool only on equal prefixes.
// Every key with count >= T is in C, so max(C) is the global max whenever it is >= T;
// otherwise (or when C has bloated) the host rebuilds C with a fresh T.  Zero-count keys that
// are still present are the reference's leftover dict keys; once no positive count remains
// (every word is one token) the reference pops them in descending byte order, which the host
// reproduces.
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <unordered_map>

#include "internal.h"
#include "prims.h"
#include "train_state.h"
#include "train_round.h"
#include "train_select.h"
#include "train_merge.h"
#include "train_apply.h"
#include "train_setup.h"

namespace bpe {

namespace {

// ------------------------------------------------------------------ host driver
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

template <class TokT>
struct HostWords {   // owns the device arrays behind a WordsDev
    DevBuf<TokT> slot[kNumCls];
    DevBuf<unsigned long long> cnt[kNumCls];
    unsigned n[kNumCls] = {0, 0, 0, 0};
    DevBuf<TokT> ltok;
    DevBuf<unsigned long long> lbeg, lcnt;
    DevBuf<uint32_t> llen;
    unsigned ln = 0;
    unsigned total() const { return n[0] + n[1] + n[2] + n[3] + ln; }
    WordsDev<TokT> dev() const {
        WordsDev<TokT> W{};
        for (int c = 0; c < kNumCls; ++c) W.c[c] = SlotCls<TokT>{slot[c].p, cnt[c].p, n[c], 0, 0, 0};
        W.ltok = ltok.p; W.lbeg = lbeg.p; W.llen = llen.p; W.lcnt = lcnt.p; W.ln = ln;
        return W;
    }
};

template <class TokT>
class MergeLoop {
   public:
    MergeLoop(hipStream_t stream, Comm* comm, const uint8_t* text, int n_rounds, TrainOutput& out)
        : s_(stream), comm_(comm), text_(text), n_rounds_(n_rounds), out_(out) {}
    ~MergeLoop() {
        if (snap_st_) (void)hipHostFree(snap_st_);
        if (snap_ti_) (void)hipHostFree(snap_ti_);
        for (auto e : blk_ev_)
            if (e) (void)hipEventDestroy(e);
    }
    MergeLoop(const MergeLoop&) = delete;
    MergeLoop& operator=(const MergeLoop&) = delete;

    void build_words(const WordCounts& wc, const std::vector<std::string>& specials);
    void run();

   private:
    static constexpr int kBatch = 64;
    // batched mode: [select][merge][apply] trips per block; a halt leaves at most ~1.5 blocks of
    // empty trips queued behind it (8-16 give 260-262 ms of merges, 32 263-266:
    // profiles/r03/o_trips_sweep.txt)
    static constexpr int kTrips = 8;
    static_assert(2 * kTrips <= kBatch, "two blocks' timing events fit the event pool");
    static constexpr int kArgBlocks = 64;
    static constexpr unsigned kCScanBlocks = 64;   // k_apply_argmax workgroups scanning C
    unsigned nparts_ = 0;                          // argmax partials the next k_merge reduces
    static constexpr int kTimingStride = 8;   // k_merge launches timed: one in 8
    static constexpr unsigned long long kTarget = 4096;
    // batched mode: the pair table grows past load 1 / kPairLoadDiv (an insert is an unsuccessful
    // linear-probe search: ~2.5 dependent probes at load 1/2, ~1.4 at 1/4)
    static constexpr size_t kPairLoadDiv = 2;   // 4 measured: no gain (366 vs 364 ms)

    void alloc_pairs(size_t cap);
    void grow_pairs();
    void ensure_pool(unsigned need);
    void push_state() { BPE_HIP(hipMemcpyAsync(st_.p, &hs_, sizeof(hs_), hipMemcpyHostToDevice, s_)); }
    void pull_state() {
        BPE_HIP(hipMemcpyAsync(&hs_, st_.p, sizeof(hs_), hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
    }
    int rebuild();  // 0 ok, 1 exhausted (only zero-count keys), 2 empty
    void exhaustion();
    void compact();
    void layout_blocks();
    void build_index();
    PairsDev pairs() const { return PairsDev{pkey_.p, pcnt_.p, pflag_.p, pcap_ - 1, C_.p}; }
    ToksDev toks() const {
        return ToksDev{pool_.p, toff_.p, tlen_.p, thash_.p, tpw_.p, tkey8_.p, tmap_.p,
                       (uint32_t)(tmap_.n - 1)};
    }

    hipStream_t s_;
    Comm* comm_;
    // the sharded exchange runs when there are several ranks; BPE355_FORCE_COMM=1 runs it on a
    // 1-rank communicator too (tests the RCCL calls on a single-GPU box)
    bool sharded() const {
        static const bool force = std::getenv("BPE355_FORCE_COMM") != nullptr;
        return comm_ && (comm_->nranks > 1 || force);
    }
    const uint8_t* text_;
    int n_rounds_;
    TrainOutput& out_;

    RoundState hs_{};
    DevBuf<RoundState> st_;
    // words
    unsigned n_words_ = 0, max_len_ = 0;
    HostWords<TokT> words_;
    WordsDev<TokT> wdev_{};
    WordsDev<TokT> wdev_trip_{};    // the slot classes over k_trip's workgroups
    unsigned trip_grid_ = 1;
    unsigned merge_grid_ = 1;
    double scan_bytes_ = 0, long_bytes_ = 0;
    unsigned long long long_tokens_ = 0;
    unsigned n_live_ = 0;
    DevBuf<unsigned long long> hist_;
    // pairs
    size_t pcap_ = 0;
    DevBuf<unsigned long long> pkey_;
    DevBuf<long long> pcnt_;
    DevBuf<unsigned> pflag_;
    DevBuf<uint4> C_;
    // tokens
    unsigned tok_cap_ = 0;
    size_t lr_member_ = 0;        // cells per member: 2 x tok_cap_, rounded up to whole 64-cell blocks
    DevBuf<unsigned> tb_, tbc_;   // touched-block bitmaps (CellMarks)
    CellMarks cm_{};
    DevBuf<uint8_t> pool_;
    DevBuf<uint32_t> toff_, tlen_;
    DevBuf<unsigned long long> tmap_;
    DevBuf<unsigned long long> thash_, tpw_, tkey8_;
    DevBuf<unsigned long long> LR_;
    DevBuf<Partial> part_;
    DevBuf<uint32_t> m_a_, m_b_, m_new_, m_mode_;
    // batched rounds (single rank): several exact merges per trip (k_select)
    bool batched_ = false;
    bool fused_ = false;         // k_trip (BPE355_FOLD=1), else k_select + k_merge_batch
    int max_batch_ = kMaxBatch;
    long long trips_launched_ = 0, trips_run_ = 0, rounds_batched_ = 0;
    std::unique_ptr<std::vector<int>> trip_log_;   // analysis knob BPE355_TRIP_LOG=path: every trip's record
    DevBuf<BatchState> bs_;
    DevBuf<Batch> batch_;
    DevBuf<unsigned long long> dbg_, sig_;   // BPE355_CHECK_MARKS
    DevBuf<uint32_t> tags_;      // per slot word: the last batch that claimed it
    DevBuf<int> trip_info_;      // per trip of a block: first round, members, scan mode, list entries (2 slots)
    RoundState* snap_st_ = nullptr;   // pinned: the state at the end of each in-flight block
    int* snap_ti_ = nullptr;          // pinned: each block's trip_info
    RoundState* snap_st_dev_ = nullptr;   // (their device-side addresses)
    int* snap_ti_dev_ = nullptr;
    hipEvent_t blk_ev_[2] = {nullptr, nullptr};
    long long slot_base_[2] = {0, 0};   // trips launched before each slot's block
    void launch_block(int slot, bool timing, std::vector<hipEvent_t>& ev);
    void finish_block(int slot, bool timing, std::vector<hipEvent_t>& ev, double& k1_ms, double& k1_bytes,
                      long long& k1_launches);
    DevBuf<unsigned long long> probe_;   // BPE355_PROBE stamps
    void report_probe();
    DevBuf<Partial> list_;       // the candidate list (every present key >= T2)
    static constexpr unsigned kApplyBatchBlocks = kApplyGrid;
    void reset_tags();

    DevBuf<long long> m_cnt_;   // BPE355_ROUND_LOG: each round's winning count (else unallocated)
    DevBuf<RebuildStats> rs_;
    // posting index
    DevBuf<uint32_t> ilist_, ibeg_, ilen_;
    DevBuf<uint32_t> ix_cnt_, ix_pos_, ix_keys_, ix_vals_, ix_keys2_;   // its build's scratch
    DevBuf<uint8_t> ix_tmp_;
    HostWords<TokT> spare_;   // the word table's other buffer set (compaction writes into it)
    unsigned cls_cap_[kNumCls] = {};   // words each slot class can ever hold (set by the first compaction)
    bool cls_cap_set_ = false;
    DevBuf<MoveCounts> move_counts_;
    DevBuf<unsigned> move_blk_;
    IndexDev idev_{};
    int next_index_round_ = 256;
};

template <class TokT>
void MergeLoop<TokT>::build_words(const WordCounts& wc, const std::vector<std::string>& specials) {
    // specials -> device (compared once per unique word, not per occurrence)
    std::string spb;
    std::vector<uint32_t> spo, spl;
    for (const auto& s : specials) { spo.push_back((uint32_t)spb.size()); spl.push_back((uint32_t)s.size()); spb += s; }
    DevBuf<uint8_t> d_spb(std::max<size_t>(spb.size(), 1));
    DevBuf<uint32_t> d_spo(std::max<size_t>(spo.size(), 1)), d_spl(std::max<size_t>(spl.size(), 1));
    if (!spb.empty()) BPE_HIP(hipMemcpyAsync(d_spb.p, spb.data(), spb.size(), hipMemcpyHostToDevice, s_));
    if (!spo.empty()) {
        BPE_HIP(hipMemcpyAsync(d_spo.p, spo.data(), spo.size() * 4, hipMemcpyHostToDevice, s_));
        BPE_HIP(hipMemcpyAsync(d_spl.p, spl.data(), spl.size() * 4, hipMemcpyHostToDevice, s_));
    }
    // occupied count-table slots -> (offset, len, count) records
    DevBuf<unsigned> cnts(2);
    BPE_HIP(hipMemsetAsync(cnts.p, 0, 8, s_));
    DevBuf<unsigned long long> w_off(wc.cap), w_cnt(wc.cap);
    DevBuf<uint32_t> w_len(wc.cap);
    hipLaunchKernelGGL(k_collect_words, dim3(ceil_div(wc.cap, (size_t)kCollectThreads * kCollectPer)),
                       dim3(kCollectThreads), 0, s_, wc.kv.p,
                       wc.pos.p, wc.cap, text_, d_spb.p, d_spo.p, d_spl.p, (int)specials.size(),
                       w_off.p, w_len.p, w_cnt.p, cnts.p, cnts.p + 1);
    BPE_HIP(hipGetLastError());
    unsigned h2[2];
    BPE_HIP(hipMemcpyAsync(h2, cnts.p, 8, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    n_words_ = h2[0];
    max_len_ = h2[1];
    const unsigned n = n_words_;
    hist_.alloc((size_t)kHistReplicas * 65536);
    BPE_HIP(hipMemsetAsync(hist_.p, 0, hist_.bytes(), s_));
    // all words start in the CSR side table; compact() then sorts them into slot classes
    HostWords<TokT>& H = words_;
    unsigned long long total_tok = 0;
    H.ln = n;
    H.llen.alloc(std::max(n, 1u));
    H.lbeg.alloc(std::max(n, 1u));
    H.lcnt.alloc(std::max(n, 1u));
    if (n) {
        DevBuf<unsigned long long> len64(n);
        hipLaunchKernelGGL(k_len_u64, dim3(ceil_div(n, 256)), dim3(256), 0, s_, w_len.p, n, len64.p);
        exclusive_sum(len64.p, H.lbeg.p, n, s_);
        unsigned long long last[2];
        BPE_HIP(hipMemcpyAsync(&last[0], H.lbeg.p + n - 1, 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(&last[1], len64.p + n - 1, 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        total_tok = last[0] + last[1];
    }
    H.ltok.alloc(std::max<unsigned long long>(total_tok, 1));
    if (n) {
        BPE_HIP(hipMemcpyAsync(H.llen.p, w_len.p, n * 4ull, hipMemcpyDeviceToDevice, s_));
        BPE_HIP(hipMemcpyAsync(H.lcnt.p, w_cnt.p, n * 8ull, hipMemcpyDeviceToDevice, s_));
        hipLaunchKernelGGL(k_fill_words<TokT>, dim3(ceil_div(n, 256)), dim3(256), 0, s_, text_, w_off.p,
                           w_len.p, H.lbeg.p, n, H.ltok.p);
        hipLaunchKernelGGL(k_hist_words, dim3(ceil_div(n, 256)), dim3(256), 0, s_, w_off.p,
                           w_len.p, w_cnt.p, text_, n, hist_.p);
        BPE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_hist_reduce, dim3(256), dim3(256), 0, s_, hist_.p);
    out_.stats.n_words = n;
    out_.stats.n_word_tokens = (int64_t)total_tok;
    BPE_HIP(hipStreamSynchronize(s_));
    n_live_ = n;
    compact();
}

// Rewrite the word table: drop words of one id, move every word to the narrowest slot class.
template <class TokT>
void MergeLoop<TokT>::compact() {
    HostWords<TokT>& H = words_;
    const unsigned total = H.total();
    DevBuf<MoveCounts>& mc = move_counts_;
    DevBuf<unsigned>& blk = move_blk_;
    mc.reserve(1);
    blk.reserve((size_t)kMoveBlocks * kMoveK);
    BPE_HIP(hipMemsetAsync(mc.p, 0, sizeof(MoveCounts), s_));
    const WordsDev<TokT> src = H.dev();
    if (total) {
        hipLaunchKernelGGL(k_move_count<TokT>, dim3(kMoveBlocks), dim3(256), 0, s_, src, total, blk.p, mc.p);
        hipLaunchKernelGGL(k_move_scan, dim3(1), dim3(kMoveBlocks), 0, s_, blk.p, mc.p);
    }
    MoveCounts h{};
    BPE_HIP(hipMemcpyAsync(&h, mc.p, sizeof(h), hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    // the new table goes into the previous compaction's arrays (grow-only: the table shrinks as
    // words finish, so after the first compactions nothing is allocated or freed here)
    HostWords<TokT> D = std::move(spare_);
    // capacities: a word only ever moves to a narrower class, so class c never holds more words
    // than the first compaction put in classes >= c or in the long-word table -- sized once, the
    // arrays are never reallocated (a reallocation's free synchronised the device and cost up to
    // ~1 ms per halt; r06j: compact+index 12.1 -> 9.6 ms, merge phase 182.1 -> 179.7-180.0 ms)
    if (!cls_cap_set_) {
        unsigned ge = h.n[kNumCls];   // (long words shrink into the slot classes too)
        for (int c = kNumCls - 1; c >= 0; --c) cls_cap_[c] = ge += h.n[c];
        cls_cap_set_ = true;
    }
    for (int c = 0; c < kNumCls; ++c) {
        D.n[c] = h.n[c];
        const size_t cap = std::max(cls_cap_[c], h.n[c]);
        D.slot[c].reserve(std::max<size_t>(cap * slot_w(c), 1));
        D.cnt[c].reserve(std::max<size_t>(cap, 1));
    }
    D.ln = h.n[kNumCls];
    D.ltok.reserve(std::max<unsigned long long>(h.long_tokens, 1));
    D.lbeg.reserve(std::max(D.ln, 1u));
    D.llen.reserve(std::max(D.ln, 1u));
    D.lcnt.reserve(std::max(D.ln, 1u));
    if (total)
        hipLaunchKernelGGL(k_move<TokT>, dim3(kMoveBlocks), dim3(256), 0, s_, src, total, D.dev(), blk.p, mc.p);
    BPE_HIP(hipGetLastError());
    BPE_HIP(hipStreamSynchronize(s_));
    spare_ = std::move(words_);
    words_ = std::move(D);
    long_tokens_ = h.long_tokens;
    n_live_ = words_.total();
    hs_.n_single = 0;
    layout_blocks();
}

// Posting lists token -> words over the current slot table (long words are always scanned).
template <class TokT>
void MergeLoop<TokT>::build_index() {
    const unsigned n = wdev_.off[kNumCls];
    const unsigned tcap = 256u + (unsigned)n_rounds_ + 1u;
    if (!ibeg_.p) {
        ibeg_.alloc(tcap);
        ilen_.alloc(tcap);
    }
    BPE_HIP(hipMemsetAsync(ibeg_.p, 0, ibeg_.bytes(), s_));
    BPE_HIP(hipMemsetAsync(ilen_.p, 0, ilen_.bytes(), s_));
    unsigned long long E = 0;
    // scratch kept across builds (grow-only; the first build is the largest)
    DevBuf<uint32_t>&cnt = ix_cnt_, &pos = ix_pos_, &keys = ix_keys_, &vals = ix_vals_, &keys2 = ix_keys2_;
    DevBuf<uint8_t>& tmp = ix_tmp_;
    cnt.reserve(std::max(n, 1u));
    pos.reserve(std::max(n, 1u));
    if (n) {
        index_pass<TokT, false>(wdev_, nullptr, cnt.p, nullptr, nullptr, s_);
        exclusive_sum(cnt.p, pos.p, n, s_, &tmp);
        uint32_t last[2];
        BPE_HIP(hipMemcpyAsync(&last[0], pos.p + n - 1, 4, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(&last[1], cnt.p + n - 1, 4, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        E = (unsigned long long)last[0] + last[1];
    }
    keys.reserve(std::max<unsigned long long>(E, 1));
    vals.reserve(std::max<unsigned long long>(E, 1));
    keys2.reserve(std::max<unsigned long long>(E, 1));
    ilist_.reserve(std::max<unsigned long long>(E, 1));
    if (E) {
        index_pass<TokT, true>(wdev_, pos.p, nullptr, keys.p, vals.p, s_);
        int bits = 1;
        while ((1u << bits) < tcap) ++bits;
        radix_sort_pairs(keys.p, keys2.p, vals.p, ilist_.p, E, (unsigned)bits, s_, &tmp);
        hipLaunchKernelGGL(k_index_bounds, dim3(ceil_div(E, 256)), dim3(256), 0, s_, keys2.p, E,
                           ibeg_.p, ilen_.p);
        hipLaunchKernelGGL(k_index_lens, dim3(ceil_div(tcap, 256)), dim3(256), 0, s_, ibeg_.p, ilen_.p, tcap);
    }
    BPE_HIP(hipGetLastError());
    BPE_HIP(hipStreamSynchronize(s_));
    // scan every word when the lists pass n / 4 (r03 sweep, profiles/r03/m_full_div_sweep.txt: 2-4
    // give 258-264 ms of merges, 6 264-268, 9 275, 14 299)
    constexpr unsigned kFullDiv = 4;
    idev_ = IndexDev{ilist_.p, ibeg_.p, ilen_.p, n / kFullDiv, n};
    out_.stats.n_index_builds++;
}

// blocks of k_merge per slot class: enough waves to cover each class with a few words per
// thread in flight, block-uniform class so the scan has no per-lane class branch
template <class TokT>
void MergeLoop<TokT>::layout_blocks() {
    WordsDev<TokT> W = words_.dev();
    W.off[0] = 0;
    for (int c = 0; c < kNumCls; ++c) W.off[c + 1] = W.off[c] + W.c[c].n;
    // about one resident generation of workgroups (4 per CU): each block's prologue is a
    // chain of dependent loads, so a second generation would pay it again
    // (1024: 252.0-252.3 ms of merges against 256.3 at 768 and 258.5 at 1536)
    constexpr unsigned kGridBudget = 1024;
    double total_b = 0;
    for (int c = 0; c < kNumCls; ++c) total_b += (double)W.c[c].n * slot_w(c);
    unsigned blk = 0;
    for (int c = 0; c < kNumCls; ++c) {
        const unsigned per_thread = c == 0 ? 4 : (c == 1 ? 2 : 1);
        const unsigned need = ceil_div(W.c[c].n, 256u * per_thread);
        const unsigned share = total_b > 0 ? (unsigned)(kGridBudget * (W.c[c].n * (double)slot_w(c)) / total_b) : 0;
        W.c[c].blk0 = blk;
        W.c[c].nblk = W.c[c].n ? std::max(1u, std::min(need, share)) : 0;
        blk += W.c[c].nblk;
    }
    W.lblk0 = blk;
    W.lnblk = std::min(ceil_div(W.ln, 256u), 64u);
    blk += W.lnblk;
    merge_grid_ = std::max(blk, (unsigned)kMaxBatch);   // k_merge_batch: block j registers member j
    wdev_ = W;
    {   // k_trip's layout: the same classes over kTripThreads-thread workgroups
        constexpr unsigned r = kTripThreads / 256;
        WordsDev<TokT> Wb = W;
        unsigned bb = 0;
        for (int c = 0; c < kNumCls; ++c) {
            Wb.c[c].blk0 = bb;
            Wb.c[c].nblk = W.c[c].n ? std::max(1u, ceil_div(W.c[c].nblk, r)) : 0;
            bb += Wb.c[c].nblk;
        }
        Wb.lblk0 = bb;
        Wb.lnblk = std::min(ceil_div(W.ln, kTripThreads), 64u / r);
        bb += Wb.lnblk;
        trip_grid_ = std::max(bb, (unsigned)kMaxBatch);
        wdev_trip_ = Wb;
    }
    if (std::getenv("BPE355_TRACE"))
        std::fprintf(stderr, "[bpe355] words per slot class: %u %u %u %u, long %u (%llu ids); merge grid %u\n", W.c[0].n,
                     W.c[1].n, W.c[2].n, W.c[3].n, W.ln, (unsigned long long)long_tokens_, merge_grid_);
    // algorithmic bytes of one k_merge launch: every slot, and every long word's ids + length
    scan_bytes_ = 0;
    for (int c = 0; c < kNumCls; ++c) scan_bytes_ += (double)W.c[c].n * slot_w(c) * sizeof(TokT);
    long_bytes_ = (double)W.ln * 4 + (double)long_tokens_ * sizeof(TokT);
    scan_bytes_ += long_bytes_;
}

template <class TokT>
void MergeLoop<TokT>::alloc_pairs(size_t cap) {
    pcap_ = cap;
    pkey_.alloc(cap);
    pcnt_.alloc(cap);
    pflag_.alloc(cap);
    C_.alloc(cap);
    BPE_HIP(hipMemsetAsync(pkey_.p, 0, pkey_.bytes(), s_));
    BPE_HIP(hipMemsetAsync(pcnt_.p, 0, pcnt_.bytes(), s_));
    BPE_HIP(hipMemsetAsync(pflag_.p, 0, pflag_.bytes(), s_));
    hs_.capC = (unsigned)cap;
}

template <class TokT>
void MergeLoop<TokT>::grow_pairs() {
    DevBuf<unsigned long long> okey = std::move(pkey_);
    DevBuf<long long> ocnt = std::move(pcnt_);
    DevBuf<unsigned> oflag = std::move(pflag_);
    const size_t ocap = pcap_;
    alloc_pairs(ocap * 2);
    hs_.pair_used = 0;
    push_state();
    hipLaunchKernelGGL(k_rehash, dim3(ceil_div(ocap, 256)), dim3(256), 0, s_, okey.p, ocnt.p,
                       oflag.p, ocap, pairs(), st_.p);
    BPE_HIP(hipGetLastError());
    pull_state();
}

template <class TokT>
void MergeLoop<TokT>::ensure_pool(unsigned need) {
    if (hs_.pool_used + (unsigned long long)need <= hs_.pool_cap) return;
    unsigned long long cap = hs_.pool_cap;
    while (hs_.pool_used + (unsigned long long)need > cap) cap *= 2;
    BPE_REQUIRE(cap < (1ULL << 32), BPE_E_LIMIT, "token byte pool exceeds 4 GiB");
    DevBuf<uint8_t> np(cap);
    BPE_HIP(hipMemcpyAsync(np.p, pool_.p, hs_.pool_used, hipMemcpyDeviceToDevice, s_));
    pool_ = std::move(np);
    hs_.pool_cap = (unsigned)cap;
    push_state();
}

template <class TokT>
int MergeLoop<TokT>::rebuild() {
    out_.stats.n_rebuilds++;
    const int grid = 1024;
    BPE_HIP(hipMemsetAsync(rs_.p, 0, sizeof(RebuildStats), s_));
    hipLaunchKernelGGL(k_rebuild_hist, dim3(grid), dim3(256), 0, s_, pairs(), pcap_, rs_.p);
    BPE_HIP(hipGetLastError());
    RebuildStats h;
    BPE_HIP(hipMemcpyAsync(&h, rs_.p, sizeof(h), hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    int top = -1;
    for (int k = 63; k >= 0; --k)
        if (h.bins[k]) { top = k; break; }
    if (top < 0) return h.ghosts ? 1 : 2;
    // the log2 bin where the cumulative count from the top crosses the target
    unsigned long long cum = 0;
    int k = top;
    for (; k >= 0; --k) {
        if (cum + h.bins[k] > kTarget) break;
        cum += h.bins[k];
    }
    long long T;
    if (k < 0) {
        T = 1;
    } else {  // refine inside bin k with 1024 linear sub-bins
        const long long lo = 1LL << k, hi = lo << 1;
        const long long width = std::max(1LL, lo / 1024);
        hipLaunchKernelGGL(k_rebuild_sub, dim3(grid), dim3(256), 0, s_, pairs(), pcap_, lo, hi, width, rs_.p);
        BPE_HIP(hipGetLastError());
        BPE_HIP(hipMemcpyAsync(h.sub, rs_.p->sub, sizeof(h.sub), hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        T = hi;  // everything above bin k
        for (int j = 1023; j >= 0; --j) {
            if (!h.sub[j]) continue;
            if (cum + h.sub[j] > kTarget && cum > 0) break;
            cum += h.sub[j];
            T = lo + (long long)j * width;
            if (cum > kTarget) break;
        }
    }
    hs_.T = T;
    hs_.nC = 0;
    hs_.halt = HALT_NONE;
    push_state();
    hipLaunchKernelGGL(k_build_C, dim3(grid), dim3(256), 0, s_, pairs(), pcap_, T, st_.p);
    if (batched_) {   // the rebuilt C's best (partials) and candidate list
        BPE_HIP(hipMemsetAsync(&bs_.p->list_n[0], 0, sizeof(bs_.p->list_n), s_));
        hipLaunchKernelGGL(k_apply_batch, dim3(kApplyBatchBlocks), dim3(kApplyBatchThreads), 0, s_, st_.p, bs_.p,
                           (const Batch*)batch_.p, pairs(), toks(), LR_.p, lr_member_,
                           (size_t)kMaxBatch * lr_member_, tok_cap_, part_.p, list_.p, 1, cm_, 0);
    }
    else
        hipLaunchKernelGGL(k_argmax, dim3(kArgBlocks), dim3(256), 0, s_, st_.p, pairs(), toks(), part_.p);
    nparts_ = kArgBlocks;
    BPE_HIP(hipGetLastError());
    pull_state();
    BPE_REQUIRE(!(hs_.err & ERR_C_FULL), BPE_E_NOMEM, "candidate list overflow");
    // re-threshold when C has grown 4x (or past 16k) by crossings since this rebuild
    hs_.c_limit = (unsigned)std::min<unsigned long long>(
        std::max<unsigned long long>(4ull * hs_.nC, 4 * kTarget), hs_.capC);
    push_state();
    return 0;
}

// posting lists are rebuilt (with a compaction) when the round count has grown by this factor
// since the last build
constexpr double kIndexGrowth = 2.5;

template <class TokT>
void MergeLoop<TokT>::run() {
    st_.alloc(1);
    rs_.alloc(1);
    tok_cap_ = 256u + (unsigned)n_rounds_ + 1u;
    part_.alloc(std::max<size_t>(std::max<size_t>(kArgBlocks, kApplyBatchBlocks),
                                 ceil_div(4ull * tok_cap_, 256) + kCScanBlocks));
    // single rank: batched rounds (BPE355_BATCH = members per trip, 1..8; 0 = the per-round
    // kernels); sharded per-round exchange: the per-round kernels
    {
        const char* e = std::getenv("BPE355_BATCH");
        max_batch_ = e ? std::min(std::atoi(e), kMaxBatch) : kMaxBatch;
        batched_ = !sharded() && max_batch_ >= 1;
    }
    // cells: two buffers by round (trip) parity; batched: kMaxBatch members each
    lr_member_ = (2ull * tok_cap_ + 63) / 64 * 64;
    LR_.alloc(2 * (batched_ ? (size_t)kMaxBatch : 1) * lr_member_);
    BPE_HIP(hipMemsetAsync(LR_.p, 0, LR_.bytes(), s_));
    if (batched_) {   // touched blocks: the apply visits the dense token prefix and the marked blocks
        const unsigned dense_tok = [] {   // test knob BPE355_DENSE_TOK (>= kDenseTokMin, a multiple of 32; per call)
            const char* e = std::getenv("BPE355_DENSE_TOK");
            const unsigned v = e ? (unsigned)std::max(0, std::atoi(e)) : 2048u;
            return std::max(kDenseTokMin, v / 32 * 32);
        }();
        const unsigned tbw = ceil_div(tok_cap_, 1024u);
        const bool marks = tbw <= kTBMax && !(std::getenv("BPE355_CELL_MARKS") && std::getenv("BPE355_CELL_MARKS")[0] == '0');
        // the apply lists touched blocks once the tokens pass sparse_from (test knob
        // BPE355_SPARSE_FROM; below, scanning every cell costs less than building the list)
        const unsigned sparse_from = [&] {
            const char* e = std::getenv("BPE355_SPARSE_FROM");
            // 16384 (r06h, merge phase at the bench config, two reps: 181.3-181.9 ms, against 182.6-182.8
            // at 8192, 185.6-186.3 at 2048 and 184.5 with no marks)
            return std::max(dense_tok, e ? (unsigned)std::max(0, std::atoi(e)) : 16384u);
        }();
        cm_ = CellMarks{nullptr, nullptr, marks ? tbw : 0u, dense_tok, sparse_from, nullptr};
        if (marks) {
            tb_.alloc(2ull * kTBRep * kMaxBatch * tbw);
            tbc_.alloc((size_t)kMaxBatch * tbw);
            BPE_HIP(hipMemsetAsync(tb_.p, 0, tb_.bytes(), s_));
            BPE_HIP(hipMemsetAsync(tbc_.p, 0, tbc_.bytes(), s_));
            cm_.tb = tb_.p;
            cm_.tbc = tbc_.p;
        }
    }
    if (batched_) {
        bs_.alloc(1);
        BPE_HIP(hipMemsetAsync(bs_.p, 0, sizeof(BatchState), s_));
        batch_.alloc(1);
        BPE_HIP(hipMemsetAsync(batch_.p, 0, sizeof(Batch), s_));
        trip_info_.alloc(2 * kTI * kTrips);
        if (!snap_st_) {   // coherent pinned memory, written by k_snapshot
            BPE_HIP(hipHostMalloc(reinterpret_cast<void**>(&snap_st_), 2 * sizeof(RoundState), hipHostMallocCoherent));
            BPE_HIP(hipHostMalloc(reinterpret_cast<void**>(&snap_ti_), 2 * kTI * kTrips * sizeof(int),
                                  hipHostMallocCoherent));
            BPE_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&snap_st_dev_), snap_st_, 0));
            BPE_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&snap_ti_dev_), snap_ti_, 0));
            for (auto& e : blk_ev_) BPE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        list_.alloc(2 * kListCap);   // by trip parity
        // select and merge of a trip in one launch (k_trip), or k_select + k_merge_batch
        const char* fe = std::getenv("BPE355_FOLD");
        fused_ = fe && fe[0] == '1';
    }
    if (batched_ && std::getenv("BPE355_CHECK_MARKS")) {
        dbg_.alloc(8);
        BPE_HIP(hipMemsetAsync(dbg_.p, 0, dbg_.bytes(), s_));
        sig_.alloc(1 + kApplyBatchBlocks);
        BPE_HIP(hipMemsetAsync(sig_.p, 0, sig_.bytes(), s_));
        cm_.sig = sig_.p;
    }
    const char* trip_log_path = std::getenv("BPE355_TRIP_LOG");   // analysis knob: the trips' records
    if (batched_ && trip_log_path) trip_log_.reset(new std::vector<int>());
    m_a_.alloc(n_rounds_); m_b_.alloc(n_rounds_); m_new_.alloc(n_rounds_); m_mode_.alloc(n_rounds_);
    const char* round_log = std::getenv("BPE355_ROUND_LOG");   // analysis knob: per-round records
    if (round_log) m_cnt_.alloc(n_rounds_);
    toff_.alloc(tok_cap_); tlen_.alloc(tok_cap_);
    thash_.alloc(tok_cap_); tpw_.alloc(tok_cap_); tkey8_.alloc(tok_cap_);
    tmap_.alloc(next_pow2(16ull * tok_cap_));   // load <= 1/16: a miss (a fresh pair) is ~1 probe
    BPE_HIP(hipMemsetAsync(tmap_.p, 0, tmap_.bytes(), s_));
    const unsigned pool_cap = std::max(1u << 16, 64u * std::max(max_len_, 8u));
    pool_.alloc(pool_cap);

    // global initial pair histogram (train.py:35-49): one all-reduce when sharded; plus the
    // longest word over all ranks (a merged token can be as long as any rank's longest word)
    if (sharded()) {
        comm_->allreduce_i64(reinterpret_cast<int64_t*>(hist_.p), 65536, s_);
        std::vector<int64_t> ml(comm_->nranks, 0);
        ml[comm_->rank] = max_len_;
        DevBuf<int64_t> d_ml(ml.size());
        BPE_HIP(hipMemcpyAsync(d_ml.p, ml.data(), ml.size() * 8, hipMemcpyHostToDevice, s_));
        comm_->allreduce_i64(d_ml.p, ml.size(), s_);
        BPE_HIP(hipMemcpyAsync(ml.data(), d_ml.p, ml.size() * 8, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
        for (int64_t v : ml) max_len_ = std::max<unsigned>(max_len_, (unsigned)v);
    }
    // test knob BPE355_PAIR_CAP_LOG2: a smaller first table (>= 2^18 holds the 65 536 byte pairs
    // at load 1/2), so moderate corpora exercise grow_pairs / k_rehash as the bench corpus does
    // first table: ~2 slots per unique word (the bench corpus peaks at 0.8 keys per word, so the
    // table never grows there; each growth is a rehash plus a rebuild of C)
    int pair_log2 = 22;
    while (pair_log2 < 26 && (1ull << pair_log2) < 2ull * n_words_) ++pair_log2;
    if (const char* e = std::getenv("BPE355_PAIR_CAP_LOG2")) pair_log2 = std::max(18, std::min(30, std::atoi(e)));
    alloc_pairs(size_t(1) << pair_log2);
    const unsigned n_single_keep = hs_.n_single;
    memset(&hs_, 0, sizeof(hs_));
    hs_.n_single = n_single_keep;
    hs_.n_rounds = n_rounds_;
    hs_.ntok = 256;
    hs_.capC = (unsigned)pcap_;
    hs_.c_limit = (unsigned)pcap_;
    hs_.pool_used = 256;
    hs_.pool_cap = pool_cap;
    push_state();
    hipLaunchKernelGGL(k_init_tokens, dim3(1), dim3(256), 0, s_, toks());
    hipLaunchKernelGGL(k_init_pairs, dim3(256), dim3(256), 0, s_, hist_.p, pairs(), st_.p);
    BPE_HIP(hipGetLastError());
    pull_state();
    build_index();
    if (batched_) reset_tags();
    hs_.halt = HALT_REBUILD;
    hs_.max_len = std::max(max_len_, 1u);
    hs_.max_batch = max_batch_;
    {
        const char* e = std::getenv("BPE355_LDS_CELLS");
        hs_.narrow_limit = !(e && e[0] == '0') ? (1ll << 32) : 0;
    }
    if (batched_ && std::getenv("BPE355_PROBE") && !BPE355_PROBE_CODE)
        std::fprintf(stderr, "[bpe355 probe] BPE355_PROBE needs a library built with -DBPE355_PROBE_CODE=1 "
                             "(tools/build_variant.sh): no stamps in this one\n");
    if (batched_ && std::getenv("BPE355_PROBE") && BPE355_PROBE_CODE) {
        probe_.alloc((size_t)kProbeSlots * (n_rounds_ / kProbeTrip + 2));
        BPE_HIP(hipMemsetAsync(probe_.p, 0, probe_.bytes(), s_));
        hs_.probe = probe_.p;
    }

    const bool timing = timing_enabled();
    std::vector<hipEvent_t> ev;
    std::vector<uint32_t> hmode;
    if (timing) {
        ev.resize(2 * kBatch);
        for (auto& e : ev) BPE_HIP(hipEventCreate(&e));
    }
    double k1_ms = 0, k1_bytes = 0;
    long long k1_launches = 0;
    const bool sharded = this->sharded();

    const bool trace = std::getenv("BPE355_TRACE") != nullptr;
    const int rank = comm_ ? comm_->rank : 0;
    // host-side phase clock (trace): rebuilds, table growth, compaction + index, trip blocks
    double h_ms[4] = {0, 0, 0, 0};
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    for (;;) {
        if (trace)
            std::fprintf(stderr, "[bpe355 r%d] round %d halt %d nC %u T %lld pairs %llu err %u\n", rank,
                         hs_.round, hs_.halt, hs_.nC, hs_.T, hs_.pair_used, hs_.err);
        if (hs_.round >= n_rounds_) break;
        if (hs_.halt == HALT_REBUILD) {
            const auto t0 = now();
            const int r = rebuild();
            h_ms[0] += since(t0);
            if (r == 1) { exhaustion(); break; }
            if (r == 2) break;   // no keys left: `if len(byte_pair_frequencies) == 0: break`
        }
        if (batched_) {
            // k_select checks the pair table, the token pool and the compaction schedule before
            // every trip and hands back to the host (HALT_HOST); here the host makes room
            if (hs_.pair_used + 4ull * (hs_.ntok + kMaxBatch) * kMaxBatch > pcap_ / kPairLoadDiv) {
                const auto t0 = now();
                grow_pairs();
                h_ms[1] += since(t0);
                hs_.halt = HALT_REBUILD;   // C holds slot indices: rebuild it
                continue;
            }
            ensure_pool((unsigned)(4 * kMaxBatch) * std::max(max_len_, 1u));
            if (hs_.halt == HALT_HOST) hs_.halt = HALT_NONE;
            hs_.host_round = next_index_round_;
            hs_.single_limit = n_live_ / 4 + 1024;
            hs_.pair_limit = pcap_ / kPairLoadDiv;
            push_state();
            const auto tb0 = now();
            {   // blocks back to back until one halts; the block behind a halted one is empty
                int slot = 0;
                launch_block(slot, timing, ev);
                for (;;) {
                    launch_block(slot ^ 1, timing, ev);
                    finish_block(slot, timing, ev, k1_ms, k1_bytes, k1_launches);
                    if (hs_.halt != HALT_NONE || hs_.err) break;
                    slot ^= 1;
                }
                finish_block(slot ^ 1, timing, ev, k1_ms, k1_bytes, k1_launches);   // drained
            }
            h_ms[3] += since(tb0);
            BPE_REQUIRE(!(hs_.err & ERR_PAIRS_FULL), BPE_E_NOMEM, "pair table overflow");
            BPE_REQUIRE(!(hs_.err & ERR_C_FULL), BPE_E_NOMEM, "candidate list overflow");
            BPE_REQUIRE(!(hs_.err & ERR_POOL), BPE_E_NOMEM, "token pool overflow");
            if (hs_.halt == HALT_DONE) break;
            if (hs_.n_single > n_live_ / 4 + 1024 || hs_.round >= next_index_round_) {
                const auto t0 = now();
                compact();
                build_index();
                reset_tags();
                push_state();
                h_ms[2] += since(t0);
                next_index_round_ = std::max(hs_.round + 512, (int)(hs_.round * kIndexGrowth));
            }
            continue;
        }
        // capacity headroom for one batch (worst case: 2 new keys per token per round)
        int R = std::min(kBatch, n_rounds_ - hs_.round);
        const unsigned long long per_round = 2ull * (hs_.ntok + R + 1);
        // keep the load <= 1/2: an insert is an unsuccessful linear-probe search, ~2.5 probes at
        // load 1/2 vs ~8.5 at 3/4 -- each probe a dependent load in k_apply
        while (hs_.pair_used + per_round * R > pcap_ / 2) {
            if (R > 8) { R /= 2; continue; }
            grow_pairs();
            hs_.halt = HALT_REBUILD;   // C holds slot indices: rebuild it
            break;
        }
        if (hs_.halt == HALT_REBUILD) continue;
        ensure_pool((unsigned)R * std::max(max_len_, 1u));
        const long long start_round = hs_.round;
        for (int k = 0; k < R; ++k) {
            // rewrite -> [one all-reduce of the delta cells when sharded] -> apply -> argmax.
            // (Applying the deltas inside the merge kernel instead was measured slower: each
            // hit's pair updates serialize on one thread, see DESIGN.md.)  With timing on, one
            // launch in kTimingStride is timed, by events stamped from k_merge's own dispatch
            // packet (events on every launch cost ~8 us of idle per round).
            const bool timed = timing && (start_round + k) % kTimingStride == 0;
            // the round's cells: buffer (round & 1); k_apply_argmax clears the other one
            const long long rnd = start_round + k;
            unsigned long long* LRc = LR_.p + (size_t)(rnd & 1) * 2 * tok_cap_;
            unsigned long long* LRo = LR_.p + (size_t)((rnd + 1) & 1) * 2 * tok_cap_;
            hipExtLaunchKernelGGL(k_merge<TokT>, dim3(merge_grid_), dim3(256), 0, s_,
                                  timed ? ev[2 * k] : nullptr, timed ? ev[2 * k + 1] : nullptr, 0,
                                  st_.p, (const Partial*)part_.p, (int)nparts_, pairs(), toks(),
                                  wdev_, idev_, LRc, m_a_.p, m_b_.p, m_new_.p, m_mode_.p, m_cnt_.p);
            if (sharded) {   // the one collective per merge round
                const size_t ntok_bound = 256 + (size_t)rnd + 1;
                comm_->allreduce_i64(reinterpret_cast<int64_t*>(LRc), 2 * ntok_bound, s_);
            }
            const unsigned ntb = 256u + (unsigned)rnd + 1u;
            const unsigned cell_blocks = ceil_div(4ull * ntb, kApplyThreads);
            const unsigned c_blocks = std::min<unsigned>(kCScanBlocks,
                                                         std::max(1u, ceil_div(hs_.c_limit, kApplyThreads)));
            hipLaunchKernelGGL(k_apply_argmax, dim3(cell_blocks + c_blocks), dim3(kApplyThreads), 0, s_, st_.p,
                               pairs(), toks(), (const unsigned long long*)LRc, LRo, ntb, cell_blocks,
                               part_.p);
            nparts_ = cell_blocks + c_blocks;
        }
        BPE_HIP(hipGetLastError());
        pull_state();
        if (timing) {
            const int done = (int)(hs_.round - start_round);
            hmode.resize(std::max(done, 1));
            if (done)
                BPE_HIP(hipMemcpy(hmode.data(), m_mode_.p + start_round, done * 4ull, hipMemcpyDeviceToHost));
            const double slot_avg = scan_bytes_ / std::max(1u, idev_.n_slot_words + words_.ln);
            for (int k = 0; k < std::min(done, R); ++k) {
                if ((start_round + k) % kTimingStride) continue;
                float t = 0;
                BPE_HIP(hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]));
                k1_ms += t;
                // algorithmic bytes: every slot on a full scan; list entries + their slots
                // (at the table's mean slot size) plus the long words in index mode
                k1_bytes += hmode[k] == 0xffffffffu ? scan_bytes_
                                                    : hmode[k] * (4.0 + slot_avg) + long_bytes_;
                ++k1_launches;
            }
        }
        BPE_REQUIRE(!(hs_.err & ERR_PAIRS_FULL), BPE_E_NOMEM, "pair table overflow");
        BPE_REQUIRE(!(hs_.err & ERR_C_FULL), BPE_E_NOMEM, "candidate list overflow");
        BPE_REQUIRE(!(hs_.err & ERR_POOL), BPE_E_NOMEM, "token pool overflow");
        if (hs_.halt == HALT_DONE) break;
        // compaction (drop finished words, narrower slots) + fresh posting lists: when many
        // words finished, and on a geometric schedule so later tokens get lists of their own
        if (hs_.n_single > n_live_ / 4 + 1024 || hs_.round >= next_index_round_) {
            compact();
            build_index();
            push_state();
            next_index_round_ = std::max(hs_.round + 512, (int)(hs_.round * 2.5));
        }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (trace)
        std::fprintf(stderr, "[bpe355] merge loop host clock: rebuild %.1f ms, grow %.1f, compact+index %.1f, trip blocks %.1f\n",
                     h_ms[0], h_ms[1], h_ms[2], h_ms[3]);
    if (round_log && hs_.round) {   // a, b, new, list length (~0: full scan), count per round
        const int rd = hs_.round;
        std::vector<uint32_t> va(rd), vb(rd), vn(rd), vm(rd);
        std::vector<long long> vc(rd);
        BPE_HIP(hipMemcpy(va.data(), m_a_.p, rd * 4ull, hipMemcpyDeviceToHost));
        BPE_HIP(hipMemcpy(vb.data(), m_b_.p, rd * 4ull, hipMemcpyDeviceToHost));
        BPE_HIP(hipMemcpy(vn.data(), m_new_.p, rd * 4ull, hipMemcpyDeviceToHost));
        BPE_HIP(hipMemcpy(vm.data(), m_mode_.p, rd * 4ull, hipMemcpyDeviceToHost));
        BPE_HIP(hipMemcpy(vc.data(), m_cnt_.p, rd * 8ull, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(round_log, "wb")) {
            for (int r = 0; r < rd; ++r) {
                std::fwrite(&va[r], 4, 1, f); std::fwrite(&vb[r], 4, 1, f); std::fwrite(&vn[r], 4, 1, f);
                std::fwrite(&vm[r], 4, 1, f); std::fwrite(&vc[r], 8, 1, f);
            }
            std::fclose(f);
        }
    }
    if (dbg_.p) {
        unsigned long long d[8];
        BPE_HIP(hipMemcpy(d, dbg_.p, sizeof(d), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[bpe355 check-marks] nonzero cells left after the clear: %llu (first: trip %llu member %llu "
                             "cell %llu); bitmap words left: %llu; apply workgroups with another view: %llu (first: "
                             "trip %llu workgroup %llu)\n", d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
        BPE_REQUIRE(d[0] == 0 && d[4] == 0 && d[5] == 0, BPE_E_HIP,
                    "cell marks: a delta outside the marked blocks, or apply workgroups that listed different blocks");
    }
    if (trip_log_ && !trip_log_->empty()) {   // kTI ints per trip (k > 0: the trips that ran)
        if (FILE* f = std::fopen(trip_log_path, "wb")) {
            std::fwrite(trip_log_->data(), sizeof(int), trip_log_->size(), f);
            std::fclose(f);
        }
    }
    if (probe_.p) report_probe();
    if (batched_) {
        BatchState b{};
        BPE_HIP(hipMemcpy(&b, bs_.p, sizeof(b), hipMemcpyDeviceToHost));
        out_.stats.n_trips = trips_run_;
        out_.stats.n_rounds_batched = rounds_batched_;
        if (BPE355_STATS_CODE && std::getenv("BPE355_TRACE")) {
            std::fprintf(stderr, "[bpe355] trips: list overflow %llu, head miss %llu, short %llu; k:", b.n_overflow,
                         b.n_headmiss, b.n_short);
            for (int i = 0; i <= kMaxBatch; ++i) std::fprintf(stderr, " %llu", b.k_hist[i]);
            std::fprintf(stderr, "; k=1 because: a==b %llu, not fresh %llu, no list %llu, P2 fails %llu, tie %llu\n",
                         b.k1_why[0], b.k1_why[1], b.k1_why[2], b.k1_why[3], b.k1_why[4]);
            std::fprintf(stderr, "[bpe355] batch ended by: cap %llu, list ran out %llu, candidate k failed the token "
                         "rules %llu, count gap / tie %llu, P1 alone %llu\n", b.end_why[0], b.end_why[1],
                         b.end_why[2], b.end_why[3], b.end_why[4]);
        }
    }
    out_.stats.merge_kernel_ms = k1_ms;
    out_.stats.merge_kernel_launches = k1_launches;
    out_.stats.merge_kernel_bytes = k1_bytes;
    out_.stats.n_pairs_final = (int64_t)hs_.pair_used;
    out_.stats.n_rounds_device = hs_.round;

    // pull the device decisions and replay them on the host (token bytes, dedupe check)
    const int rd = hs_.round;
    std::vector<uint32_t> ma(rd), mb(rd), mn(rd);
    if (rd) {
        BPE_HIP(hipMemcpyAsync(ma.data(), m_a_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(mb.data(), m_b_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(mn.data(), m_new_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
    }
    // (out_.merges may already hold the exhaustion tail: prepend the device rounds)
    std::vector<std::pair<std::string, std::string>> tail = std::move(out_.merges);
    out_.merges.clear();
    auto& tb = out_.tok_bytes;
    tb.clear();
    for (int b = 0; b < 256; ++b) tb.push_back(std::string(1, (char)b));
    for (int r = 0; r < rd; ++r) {
        std::string nb = tb[ma[r]] + tb[mb[r]];
        if (mn[r] == tb.size()) tb.push_back(nb);
        else BPE_REQUIRE(mn[r] < tb.size() && tb[mn[r]] == nb, BPE_E_HIP,
                         "device token dedupe disagrees with host replay");
        out_.merges.emplace_back(tb[ma[r]], tb[mb[r]]);
    }
    for (auto& m : tail) out_.merges.push_back(std::move(m));
}

// BPE355_PROBE summary (stderr): mean phase durations of the sampled trips, us
template <class TokT>
void MergeLoop<TokT>::report_probe() {
    std::vector<unsigned long long> pr(probe_.n);
    BPE_HIP(hipMemcpy(pr.data(), probe_.p, probe_.bytes(), hipMemcpyDeviceToHost));
    const char* names[] = {"sel:issue", "sel:p1+list+meta", "sel:rule", "sel:fill", "gap sel>merge", "merge:pop",
                           "merge:rewrite", "merge:flush", "gap merge>apply", "apply:clear", "apply:items",
                           "apply:blocktop", "apply:end", "gap apply>sel"};
    const int from[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
    const int to[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16};
    double acc[14] = {};
    int n = 0;
    // the last workgroups: merge flush (block 0) -> last merge workgroup done -> apply start;
    // apply end (block 0) -> last apply workgroup done -> the next trip's select start
    double tails[4] = {};
    int nt4 = 0;
    for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
        const unsigned long long* p = &pr[kProbeSlots * t];
        bool ok = true;
        for (int i = 0; i < 14; ++i) ok &= p[i] != 0;
        if (!ok) continue;
        for (int i = 0; i < 13; ++i) acc[i] += (double)(p[to[i]] - p[from[i]]) * 0.01;
        ++n;
        if (p[14] && p[15] && p[16]) {
            tails[0] += (double)(long long)(p[14] - p[8]) * 0.01;
            tails[1] += (double)(long long)(p[9] - p[14]) * 0.01;
            tails[2] += (double)(long long)(p[15] - p[13]) * 0.01;
            tails[3] += (double)(long long)(p[16] - p[15]) * 0.01;
            ++nt4;
        }
    }
    std::fprintf(stderr, "[bpe355 probe] %d sampled trips, mean us:", n);
    for (int i = 0; i < 13 && n; ++i) std::fprintf(stderr, " %s %.2f |", names[i], acc[i] / n);
    std::fprintf(stderr, "\n");
    {   // inside select's rule: p1 over the waves | list head + metadata | clash + k | strict gap / 4'
        double r[4] = {};
        int nr = 0;
        for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
            const unsigned long long* p = &pr[kProbeSlots * t];
            if (!(p[2] && p[17] && p[18] && p[19] && p[3])) continue;
            r[0] += (double)(p[17] - p[2]) * 0.01; r[1] += (double)(p[18] - p[17]) * 0.01;
            r[2] += (double)(p[19] - p[18]) * 0.01; r[3] += (double)(p[3] - p[19]) * 0.01;
            ++nr;
        }
        if (nr)
            std::fprintf(stderr, "[bpe355 probe] select rule: p1 %.2f | head+meta %.2f | clash+k+gap %.2f | record %.2f\n",
                         r[0] / nr, r[1] / nr, r[2] / nr, r[3] / nr);
        double q[6] = {};
        int nq = 0;
        for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
            const unsigned long long* p = &pr[kProbeSlots * t];
            if (!p[1] || !p[24] || !p[25] || !p[26] || !p[27] || !p[28] || !p[2]) continue;
            q[0] += (double)((long long)p[24] - (long long)p[1]) * 0.01; q[1] += (double)((long long)p[25] - (long long)p[24]) * 0.01;
            q[2] += (double)((long long)p[26] - (long long)p[1]) * 0.01; q[3] += (double)((long long)p[27] - (long long)p[25]) * 0.01;
            q[4] += (double)((long long)p[28] - (long long)p[27]) * 0.01; q[5] += (double)((long long)p[2] - (long long)p[28]) * 0.01;
            ++nq;
        }
        if (nq)
            std::fprintf(stderr, "[bpe355 probe] select phase 1 (list thread 0): list entry %.2f | metadata+dedupe %.2f | "
                                 "(wave 0 partials %.2f) | barrier %.2f | rank %.2f | minima+barrier %.2f (%d trips)\n",
                         q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq, q[4] / nq, q[5] / nq, nq);
        std::vector<double> nls, rl;
        for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
            const unsigned long long* p = &pr[kProbeSlots * t];
            if (p[30]) nls.push_back((double)p[30] - 1);
            if (p[27] && p[29]) rl.push_back(((long long)p[29] - (long long)p[27]) * 0.01);
        }
        {   // the rank stretch split: count ranks (27 -> 29), the barrier behind them (29 -> 31), the
            // exact ranking and the top entries' stores (31 -> 28)
            double a = 0, b = 0, c = 0;
            int n = 0;
            for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
                const unsigned long long* p = &pr[kProbeSlots * t];
                if (!p[27] || !p[29] || !p[31] || !p[28]) continue;
                a += ((long long)p[29] - (long long)p[27]) * 0.01;
                b += ((long long)p[31] - (long long)p[29]) * 0.01;
                c += ((long long)p[28] - (long long)p[31]) * 0.01;
                ++n;
            }
            if (n)
                std::fprintf(stderr, "[bpe355 probe] select rank: count ranks %.2f | barrier %.2f | exact rank + stores %.2f (%d trips)\n",
                             a / n, b / n, c / n, n);
        }
        std::sort(nls.begin(), nls.end());
        std::sort(rl.begin(), rl.end());
        if (!nls.empty() && !rl.empty())
            std::fprintf(stderr, "[bpe355 probe] select list entries p10 %.0f p50 %.0f p90 %.0f max %.0f | ranking loop us p50 %.2f p90 %.2f\n",
                         nls[nls.size() / 10], nls[nls.size() / 2], nls[nls.size() * 9 / 10], nls.back(),
                         rl[rl.size() / 2], rl[rl.size() * 9 / 10]);
    }
    {   // which workgroup finishes last: merge blocks below k register members; apply's last block
        int nm = 0, nm_reg = 0, na = 0, na_lastblk = 0;
        std::vector<int> mlast, alast;
        for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
            const unsigned long long* p = &pr[kProbeSlots * t];
            if (p[20]) { ++nm; nm_reg += (p[20] - 1) < kMaxBatch; mlast.push_back((int)p[20] - 1); }
            if (p[21]) { ++na; na_lastblk += (p[21] - 1) == kApplyGrid - 1; alast.push_back((int)p[21] - 1); }
        }
        if (nm && na) {
            std::sort(alast.begin(), alast.end());
            std::sort(mlast.begin(), mlast.end());
            std::fprintf(stderr, "[bpe355 probe] last merge wg < %d (registers a member): %d of %d (median wg %d) | "
                         "last apply wg = grid-1: %d of %d (median wg %d)\n", kMaxBatch, nm_reg, nm,
                         mlast[mlast.size() / 2], na_lastblk, na, alast[alast.size() / 2]);
            double wl = 0, wc = 0;
            for (size_t t = 0; t + 1 < pr.size() / kProbeSlots; ++t) {
                wl += (double)pr[kProbeSlots * t + 22];
                wc += (double)pr[kProbeSlots * t + 23];
            }
            std::fprintf(stderr, "[bpe355 probe] apply workgroups per trip reserving list space %.1f, C space %.1f\n",
                         wl / na, wc / na);
        }
    }
    if (nt4)
        std::fprintf(stderr, "[bpe355 probe] %d trips: merge last-workgroup tail %.2f | last merge wg > apply start %.2f | "
                     "apply last-workgroup tail %.2f | last apply wg > next select %.2f\n", nt4, tails[0] / nt4,
                     tails[1] / nt4, tails[2] / nt4, tails[3] / nt4);
    // distribution of whole trips (select start -> apply end) and of the rewrite, by trip decile
    std::vector<double> tot, rw;
    std::vector<double> dec_tot(10, 0.0), dec_rw(10, 0.0);
    std::vector<int> dec_n(10, 0);
    size_t nt = 0;   // sampled trips that ran (the buffer is sized for the worst case)
    for (size_t t = 0; t < pr.size() / kProbeSlots; ++t)
        if (pr[kProbeSlots * t] != 0) nt = t + 1;
    for (size_t t = 0; t < nt; ++t) {
        const unsigned long long* p = &pr[kProbeSlots * t];
        bool ok = true;
        for (int i = 0; i < 14; ++i) ok &= p[i] != 0;
        if (!ok) continue;
        const double a = (double)(p[13] - p[0]) * 0.01, b = (double)(p[7] - p[6]) * 0.01;
        tot.push_back(a); rw.push_back(b);
        const size_t d = t * 10 / nt;
        dec_tot[d] += a; dec_rw[d] += b; dec_n[d]++;
    }
    auto pct = [](std::vector<double> v, double q) {
        if (v.empty()) return 0.0;
        std::sort(v.begin(), v.end());
        return v[std::min(v.size() - 1, (size_t)(q * v.size()))];
    };
    std::fprintf(stderr, "[bpe355 probe] trip us p50 %.1f p90 %.1f p99 %.1f max %.1f | rewrite p50 %.1f p90 %.1f p99 %.1f max %.1f\n",
                 pct(tot, 0.5), pct(tot, 0.9), pct(tot, 0.99), pct(tot, 1.0), pct(rw, 0.5), pct(rw, 0.9), pct(rw, 0.99),
                 pct(rw, 1.0));
    std::fprintf(stderr, "[bpe355 probe] by decile (trip/rewrite us):");
    for (int d = 0; d < 10; ++d)
        if (dec_n[d]) std::fprintf(stderr, " %.1f/%.1f", dec_tot[d] / dec_n[d], dec_rw[d] / dec_n[d]);
    std::fprintf(stderr, "\n");
}

template <class TokT>
void MergeLoop<TokT>::reset_tags() {
    tags_.reserve(std::max(idev_.n_slot_words, 1u));
    BPE_HIP(hipMemsetAsync(tags_.p, 0, std::max(idev_.n_slot_words, 1u) * sizeof(uint32_t), s_));
}

// One block: kTrips x [k_select][k_merge_batch][k_apply_batch], then a snapshot of the state
// and of the trips' records into pinned memory, ordered on the stream, and an event.  Two blocks
// are in flight: the host reads one block's snapshot while the next one runs, so the device does
// not idle at every host check.  A block launched after a halt finds nothing to do (k_select
// sees st->halt).  With timing on, k_merge_batch is event-timed on one trip in kTimingStride
// (events stamped by its own dispatch packet).
template <class TokT>
void MergeLoop<TokT>::launch_block(int slot, bool timing, std::vector<hipEvent_t>& ev) {
    const size_t lr_member = lr_member_, lr_parity = (size_t)kMaxBatch * lr_member;
    const unsigned ntb = tok_cap_;
    const unsigned apply_blocks = kApplyBatchBlocks;
    // whether this block's applies may list touched blocks: the tokens may pass cm_.sparse_from
    // within the two blocks in flight (the apply decides from the batch's own count)
    const int sparse_hint = cm_.tbw && (long long)hs_.ntok + 2ll * kTrips * kMaxBatch >= (long long)cm_.sparse_from;
    int* ti = trip_info_.p + (size_t)slot * kTI * kTrips;
    slot_base_[slot] = trips_launched_;
    for (int t = 0; t < kTrips; ++t) {
        const bool timed = timing && (trips_launched_ + t) % kTimingStride == 0;
        hipEvent_t* e = &ev[2 * ((size_t)slot * kTrips + t)];
        const SelOut so{m_a_.p, m_b_.p, m_new_.p, m_mode_.p, m_cnt_.p, ti, t};
        if (fused_ && sizeof(TokT) == 2) {   // (u32 ids: k_trip would spill at 1024 threads)
            hipExtLaunchKernelGGL(k_trip<TokT>, dim3(trip_grid_), dim3(kTripThreads), 0, s_,
                                  timed ? e[0] : nullptr, timed ? e[1] : nullptr, 0,
                                  st_.p, bs_.p, pairs(), toks(), wdev_trip_, idev_, batch_.p, (const Partial*)part_.p,
                                  (const Partial*)list_.p, so, LR_.p, lr_member, lr_parity, tags_.p, cm_);
        } else {
            hipLaunchKernelGGL(k_select, dim3(1), dim3(kSelThreads), 0, s_, (const RoundState*)st_.p, bs_.p, toks(),
                               idev_, batch_.p, (const Partial*)part_.p, (const Partial*)list_.p, so);
            hipExtLaunchKernelGGL(k_merge_batch<TokT>, dim3(merge_grid_), dim3(256), 0, s_,
                                  timed ? e[0] : nullptr, timed ? e[1] : nullptr, 0,
                                  st_.p, (const Batch*)batch_.p, pairs(), toks(), wdev_, idev_, LR_.p, lr_member,
                                  lr_parity, tags_.p, cm_);
        }
        if (dbg_.p)
            hipLaunchKernelGGL(k_check_clear, dim3(256), dim3(256), 0, s_, (const Batch*)batch_.p, (const unsigned long long*)LR_.p,
                               lr_member, lr_parity, (const unsigned*)cm_.tb, cm_.tbw, dbg_.p);
        hipLaunchKernelGGL(k_apply_batch, dim3(apply_blocks), dim3(kApplyBatchThreads), 0, s_, st_.p, bs_.p,
                           (const Batch*)batch_.p, pairs(), toks(), LR_.p, lr_member, lr_parity, ntb, part_.p,
                           list_.p, 0, cm_, sparse_hint);
        if (sig_.p)
            hipLaunchKernelGGL(k_check_sig, dim3(1), dim3(256), 0, s_, (const Batch*)batch_.p, sig_.p,
                               (unsigned)kApplyBatchBlocks, dbg_.p);
    }
    static_assert(sizeof(RoundState) % 4 == 0, "k_snapshot copies words");
    // the block's snapshot: one small kernel stores the state and the trip records into pinned
    // host memory (two copy packets cost ~3x as much at every block boundary)
    hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(256), 0, s_, (const uint32_t*)st_.p,
                       (unsigned)(sizeof(RoundState) / 4), (const uint32_t*)ti, (unsigned)(kTI * kTrips),
                       (uint32_t*)(snap_st_dev_ + slot), (uint32_t*)(snap_ti_dev_ + (size_t)slot * kTI * kTrips));
    BPE_HIP(hipGetLastError());
    BPE_HIP(hipEventRecord(blk_ev_[slot], s_));
    trips_launched_ += kTrips;
}

template <class TokT>
void MergeLoop<TokT>::finish_block(int slot, bool timing, std::vector<hipEvent_t>& ev, double& k1_ms,
                                   double& k1_bytes, long long& k1_launches) {
    BPE_HIP(hipEventSynchronize(blk_ev_[slot]));
    hs_ = snap_st_[slot];
    const int* ti = snap_ti_ + (size_t)slot * kTI * kTrips;
    for (int t = 0; t < kTrips; ++t) {
        trips_run_ += ti[kTI * t + 1] > 0;
        rounds_batched_ += ti[kTI * t + 1] > 1 ? ti[kTI * t + 1] : 0;
        if (trip_log_) trip_log_->insert(trip_log_->end(), ti + kTI * t, ti + kTI * (t + 1));
    }
    if (!timing) return;
    const double slot_avg = scan_bytes_ / std::max(1u, idev_.n_slot_words + words_.ln);
    for (int t = 0; t < kTrips; ++t) {
        if ((slot_base_[slot] + t) % kTimingStride || ti[kTI * t + 1] <= 0) continue;
        float ms = 0;
        const hipEvent_t* e = &ev[2 * ((size_t)slot * kTrips + t)];
        BPE_HIP(hipEventElapsedTime(&ms, e[0], e[1]));
        // algorithmic bytes: every slot on a full scan, else the members' list entries and their
        // slots (at the table's mean slot size); every long word once per trip
        const bool full = ti[kTI * t + 2] != 0;
        k1_ms += ms;
        k1_bytes += full ? scan_bytes_ : long_bytes_ + (double)(unsigned)ti[kTI * t + 3] * (4.0 + slot_avg);
        ++k1_launches;
    }
}

// Every word is one token: the reference keeps popping the remaining zero-count keys,
// greatest (bytes a, bytes b) first, until the rounds run out or the dict is empty.
template <class TokT>
void MergeLoop<TokT>::exhaustion() {
    const int rd = hs_.round;
    std::vector<uint32_t> ma(rd), mb(rd), mn(rd);
    if (rd) {
        BPE_HIP(hipMemcpyAsync(ma.data(), m_a_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(mb.data(), m_b_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipMemcpyAsync(mn.data(), m_new_.p, rd * 4ull, hipMemcpyDeviceToHost, s_));
    }
    DevBuf<unsigned long long> keys(std::max<size_t>(hs_.pair_used, 1));
    DevBuf<unsigned> nk(1);
    BPE_HIP(hipMemsetAsync(nk.p, 0, 4, s_));
    hipLaunchKernelGGL(k_collect_present, dim3(1024), dim3(256), 0, s_, pairs(), pcap_, keys.p, nk.p);
    unsigned hk = 0;
    BPE_HIP(hipMemcpyAsync(&hk, nk.p, 4, hipMemcpyDeviceToHost, s_));
    BPE_HIP(hipStreamSynchronize(s_));
    std::vector<unsigned long long> hkeys(hk);
    if (hk) {
        BPE_HIP(hipMemcpyAsync(hkeys.data(), keys.p, hk * 8ull, hipMemcpyDeviceToHost, s_));
        BPE_HIP(hipStreamSynchronize(s_));
    }
    std::vector<std::string> tb;
    for (int b = 0; b < 256; ++b) tb.push_back(std::string(1, (char)b));
    for (int r = 0; r < rd; ++r) {
        std::string nb = tb[ma[r]] + tb[mb[r]];
        if (mn[r] == tb.size()) tb.push_back(nb);
        else BPE_REQUIRE(mn[r] < tb.size() && tb[mn[r]] == nb, BPE_E_HIP,
                         "device token dedupe disagrees with host replay");
    }
    std::vector<std::pair<std::string, std::string>> ghosts;
    ghosts.reserve(hk);
    for (auto k : hkeys) ghosts.emplace_back(tb[k >> 32], tb[k & 0xffffffffu]);
    std::sort(ghosts.begin(), ghosts.end(), [](const auto& x, const auto& y) { return x > y; });
    const size_t left = (size_t)(n_rounds_ - rd);
    if (ghosts.size() > left) ghosts.resize(left);
    out_.stats.n_rounds_host = (int64_t)ghosts.size();
    out_.merges = std::move(ghosts);   // the tail; run() prepends the device rounds
}

}  // namespace

namespace {

// Several ranks: an error one rank met before the first collective (reading or validating its
// slab) is raised by every rank, so none waits in a collective another never reaches.  The
// error of the earliest slab wins; a UTF-8 position is reported in whole-corpus bytes.
void agree_on_errors(Comm* comm, const Error* mine, hipStream_t stream) {
    const int R = comm->nranks;
    std::vector<int64_t> v(3 * (size_t)R, 0);
    if (mine) {
        v[3 * comm->rank] = mine->code;
        v[3 * comm->rank + 1] = mine->sys_errno;
        const size_t p = mine->msg.find("position ");
        v[3 * comm->rank + 2] = p == std::string::npos ? 0 : std::stoll(mine->msg.substr(p + 9));
    }
    DevBuf<int64_t> d(v.size());
    BPE_HIP(hipMemcpyAsync(d.p, v.data(), v.size() * 8, hipMemcpyHostToDevice, stream));
    comm->allreduce_i64(d.p, v.size(), stream);
    BPE_HIP(hipMemcpyAsync(v.data(), d.p, v.size() * 8, hipMemcpyDeviceToHost, stream));
    BPE_HIP(hipStreamSynchronize(stream));
    for (int r = 0; r < R; ++r) {
        const int code = (int)v[3 * r];
        if (!code) continue;
        if (r == comm->rank && mine) throw *mine;
        if (code == BPE_E_UTF8)
            throw Error{code, "'utf-8' codec can't decode byte at position " + std::to_string(v[3 * r + 2])};
        throw Error{code, "rank " + std::to_string(r) + " failed before training (code " + std::to_string(code) + ")",
                    (int)v[3 * r + 1]};
    }
}

}  // namespace

bool per_round_exchange() {
    const char* ex = std::getenv("BPE355_EXCHANGE");
    return ex && std::string(ex) == "rounds";
}

void train_on_device(const uint8_t* d_raw, size_t n, int vocab_size,
                     const std::vector<std::string>& specials, Comm* comm, hipStream_t stream,
                     TrainOutput& out, const TrainOpts& opt, Prepared* pre) {
    const auto t0 = std::chrono::steady_clock::now();
    out = TrainOutput{};
    DevBuf<uint8_t> scratch;
    size_t tn = 0;
    const uint8_t* text = nullptr;
    const bool several = comm && comm->nranks > 1;
    WordCounts wc;
    float count_ms = 0;
    std::chrono::steady_clock::time_point t1;
    {
        Error err{0, ""};
        bool failed = opt.has_pending;
        if (failed) err = opt.pending;
        if (!failed && pre) {   // validated and counted while the corpus arrived (drive.hip)
            text = pre->text;
            tn = pre->n;
            wc = std::move(pre->wc);
            count_ms = pre->count_kernel_ms;
            out.stats.t_prepare_ms = pre->t_prepare_ms;
            out.stats.n_bytes = (int64_t)tn;
            t1 = std::chrono::steady_clock::now() - std::chrono::duration_cast<std::chrono::steady_clock::duration>(
                                                         std::chrono::duration<double, std::milli>(pre->t_count_ms));
        } else if (!failed) {
            try {
                text = prepare_text(d_raw, n, scratch, &tn, stream);
                out.stats.t_prepare_ms = ms_since(t0);
                out.stats.n_bytes = (int64_t)tn;
                t1 = std::chrono::steady_clock::now();
                count_words(text, tn, wc, stream, timing_enabled() ? &count_ms : nullptr);
            } catch (const Error& e) {
                if (!several && !opt.slab_offset) throw;
                err = e;
                failed = true;
            }
        }
        if (failed && err.code == BPE_E_UTF8 && opt.slab_offset) {
            const size_t p = err.msg.find("position ");
            if (p != std::string::npos)
                err.msg = "'utf-8' codec can't decode byte at position " +
                          std::to_string(std::stoull(err.msg.substr(p + 9)) + opt.slab_offset);
        }
        if (several) agree_on_errors(comm, failed ? &err : nullptr, stream);
        else if (failed) throw err;
    }

    const long long rounds = merge_rounds(vocab_size, specials);

    out.stats.t_count_ms = ms_since(t1);
    out.stats.count_kernel_ms = count_ms;
    out.stats.count_kernel_bytes = (double)tn;
    out.stats.n_pretokens = (int64_t)wc.n_pretokens;
    out.stats.n_count_records = (int64_t)wc.n_records;
    out.stats.count_reduce_ms = wc.reduce_ms;
    out.stats.count_partial_ms = wc.partial_ms;
    out.stats.n_count_batches = (int64_t)wc.batches;
    if (rounds <= 0) {
        out.stats.t_total_ms = ms_since(t0);
        return;
    }
    BPE_REQUIRE(rounds < (1LL << 31) - 512, BPE_E_LIMIT, "vocab_size too large");
    // several ranks: by default exchange the word tables once and train on their union with no
    // per-round collective (exchange.hip); BPE355_EXCHANGE=rounds keeps the slabs' words local and
    // all-reduces the pair deltas every round.  BPE355_FORCE_EXCHANGE=1 runs the word exchange
    // on a 1-rank communicator too (tests the collective on a single-GPU box).
    DevBuf<uint8_t> union_text;
    Comm* loop_comm = comm;
    const bool per_round = per_round_exchange();
    if (comm && !per_round && (comm->nranks > 1 || std::getenv("BPE355_FORCE_EXCHANGE"))) {
        auto te = std::chrono::steady_clock::now();
        uint64_t uw = 0;
        union_word_tables(text, wc, comm, stream, union_text, &uw, &out.stats);
        text = union_text.p;
        loop_comm = nullptr;
        out.stats.t_exchange_ms = ms_since(te);
        out.stats.n_exchanged_words = (int64_t)uw;
    }
    if (!opt.merge_loop) {
        out.stats.t_total_ms = ms_since(t0);
        return;
    }
    train_words(text, wc, vocab_size, specials, stream, out, loop_comm, &wc);
    out.stats.t_total_ms = ms_since(t0);
}

long long merge_rounds(int vocab_size, const std::vector<std::string>& specials) {
    // len(vocab) at loop start: Vocab(special_tokens) = specials then the 256 bytes, deduped
    std::set<std::string> base;
    for (const auto& s : specials) base.insert(s);
    for (int b = 0; b < 256; ++b) base.insert(std::string(1, (char)b));
    return (long long)vocab_size - (long long)base.size();
}

void train_words(const uint8_t* text, const WordCounts& wc, int vocab_size, const std::vector<std::string>& specials,
                 hipStream_t stream, TrainOutput& out, Comm* loop_comm, WordCounts* drop_after_build) {
    const long long rounds = merge_rounds(vocab_size, specials);
    if (rounds <= 0) return;
    BPE_REQUIRE(rounds < (1LL << 31) - 512, BPE_E_LIMIT, "vocab_size too large");
    auto go = [&](auto tag) {
        using TokT = decltype(tag);
        auto t2 = std::chrono::steady_clock::now();
        MergeLoop<TokT> loop(stream, loop_comm, text, (int)rounds, out);
        loop.build_words(wc, specials);
        if (drop_after_build) { WordCounts drop = std::move(*drop_after_build); }
        out.stats.t_words_ms = ms_since(t2);
        auto t3 = std::chrono::steady_clock::now();
        loop.run();
        out.stats.t_merge_ms = ms_since(t3);
    };
    if (256 + rounds + 1 < 65535) go(uint16_t{});
    else go(uint32_t{});
}

}  // namespace bpe
