// Encode with BPE-dropout (Provilkov et al., 2020): every candidate merge of every pre-token
// occurrence is skipped with probability thr / 2^24, drawn from a counter-based generator, so the
// ids of a document depend on (seed, doc_key, text) alone.
//
//   wk      = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ doc_key) ^ off)    per pre-token; off:
//             the byte offset of its first byte in its document
//   dropped = (mix64(wk ^ (rnd << 32 | pos)) >> 40) < thr                       per round and pair;
//             pos: the byte offset, inside the pre-token, of the pair's left token
//   round   : the ranked adjacent pair of minimum rank among the positions not dropped; every
//             occurrence of it that is not dropped merges, left to right; none: the word is done
//
// The encoder's design (each distinct word encoded once, every occurrence a copy) does not apply:
// each occurrence draws its own merges.  encode.hip runs its front unchanged -- the segment table
// and the scan's kCuts, kPos instantiation, which leaves one record per pre-token with its first
// byte and marks the specials -- and the kernels here do the rest:
//   k_drop_merge   one lane per pre-token of up to kDropShort bytes.  Tokens, and the rank and
//                  product of every adjacent pair, live in LDS at the pre-token's byte offsets
//                  (lane-interleaved: element j of lane l at j * kDropBlock + l, one bank per lane);
//                  the live offsets are a 32-bit mask in a register, so a merge clears one bit and
//                  nothing is compacted.  A pair's rank is looked up once, and again only beside a
//                  merge.  The ids go to a pool that mirrors the text (ids <= bytes), the id count
//                  replaces the record.  Longer pre-tokens are appended to a list.
//   k_drop_long    one wave per listed pre-token, in place on the pool: a min pass and a rewrite
//                  pass per round, 64 tokens a step, the rewrite a ballot and a prefix popcount.
//   k_drop_count   per chunk, the sum of its records' id counts; one exclusive scan (prims.h)
//   k_drop_gather  per chunk, pool -> the dense ids, and every cut's id offset
//   k_drop_doc_offsets  every document's id offset from its cut
#include <algorithm>
#include <string>
#include <vector>

#include "internal.h"
#include "prims.h"

namespace bpe {
namespace {

constexpr int kDropShort = 32;      // longest pre-token of the one-lane path: one bit per byte
constexpr int kDropBlock = 128;     // 3 x 32 x 4 bytes of LDS per lane: 48 KiB per workgroup
constexpr uint32_t kNoRank = 0xffffffffu;
constexpr unsigned kDropKey = 4u;   // status: a token without a vocab id
constexpr unsigned kDropBug = 64u;  // status: a record without bytes, or a special out of range
constexpr uint32_t kDropFull = 1u << 24;

struct DropArgs {
    const uint8_t* text;
    unsigned long long n;
    size_t n_chunks, chunk;
    uint32_t* recs;
    uint32_t kind_mask, kind_special, payload_mask;
    const uint16_t* rec_pos;
    const unsigned long long* rec_base;
    const uint32_t* rec_n;
    const unsigned long long* chunk_next;
    const unsigned long long* cuts;
    const uint32_t* chunk_cut0;
    const uint32_t* cut_rec;
    const unsigned long long* cut_doc;   // per cut: the document that starts there (the last of several)
    unsigned long long doc0;             // the document of the bytes before the first cut
    uint32_t thr;
    uint64_t h_seed;                     // mix64(seed + 0x9E3779B97F4A7C15)
    uint64_t doc_base;
    uint32_t* pool;                      // n: a pre-token's ids from its first byte's index on
    uint32_t* aux;                       // n: the long path's token offsets (the caller's id buffer)
    unsigned long long* list;            // the long pre-tokens: chunk << 16 | record
    unsigned* status;                    // [0] status bits, [1] entries of list
    unsigned long long* ctot;
    const unsigned long long* coff;
    unsigned long long* cut_off;
    uint32_t* out;
};

__device__ __forceinline__ uint2 drop_rank(const DropTables& E, uint32_t a, uint32_t b) {
    const unsigned long long key = ((((unsigned long long)a) << 32) | b) + 1ULL;
    size_t s = mix64(key) & E.pm_mask;
    for (;;) {
        const unsigned long long k = E.pm_key[s];
        if (k == key) return E.pm_val[s];
        if (k == 0) return make_uint2(kNoRank, 0);
        s = (s + 1) & E.pm_mask;
    }
}

__device__ __forceinline__ bool dropped(uint64_t wk, uint32_t rnd, uint32_t pos, uint32_t thr) {
    return (uint32_t)(mix64(wk ^ (((uint64_t)rnd << 32) | pos)) >> 40) < thr;
}

struct RecGeo {
    unsigned long long pos, end;   // the record's bytes in the text
    uint64_t wk;                   // its draws' key
};
// record i of chunk c (mc records from rb on)
__device__ __forceinline__ RecGeo rec_geo(const DropArgs& A, size_t c, uint32_t i, uint32_t mc, unsigned long long rb) {
    const unsigned long long cbase = (unsigned long long)c * A.chunk;
    RecGeo g;
    g.pos = cbase + A.rec_pos[rb + i];
    g.end = i + 1 < mc ? cbase + A.rec_pos[rb + i + 1] : A.chunk_next[c];
    uint32_t lo = A.chunk_cut0[c], hi = A.chunk_cut0[c + 1];   // the cuts at or before pos: [0, lo)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (A.cuts[mid] <= g.pos) lo = mid + 1;
        else hi = mid;
    }
    const unsigned long long start = lo ? A.cuts[lo - 1] : 0ULL;
    const uint64_t doc_key = A.doc_base + (lo ? A.cut_doc[lo - 1] : A.doc0);
    g.wk = mix64(mix64(A.h_seed ^ doc_key) ^ (uint64_t)(g.pos - start));
    return g;
}

__device__ __forceinline__ bool is_special_word(const DropTables& E, const uint8_t* w, uint32_t len) {
    for (int k = 0; k < E.n_sp; ++k) {
        if (E.sp_len[k] != len) continue;
        const uint8_t* sp = E.sp_bytes + E.sp_off[k];
        uint32_t j = 0;
        while (j < len && w[j] == sp[j]) ++j;
        if (j == len) return true;
    }
    return false;
}

// One pre-token of 2..kDropShort bytes on one lane; tk, rk, pd: the lane's LDS columns (stride
// kDropBlock).  Returns its id count, the ids in out[0, count).
__device__ __forceinline__ uint32_t merge_short(const DropArgs& A, const DropTables& E, const uint8_t* w, uint32_t len,
                                                uint64_t wk, uint32_t* tk, uint32_t* rk, uint32_t* pd, uint32_t* out) {
    if (E.n_sp && is_special_word(E, w, len)) return 0;   // a pre-token equal to a special has no id
    for (uint32_t j = 0; j < len; ++j) tk[j * kDropBlock] = E.byte2tok[w[j]];
    for (uint32_t j = 0; j + 1 < len; ++j) {
        const uint2 r = drop_rank(E, tk[j * kDropBlock], tk[(j + 1) * kDropBlock]);
        rk[j * kDropBlock] = r.x;
        pd[j * kDropBlock] = r.y;
    }
    uint32_t alive = len >= 32 ? ~0u : (1u << len) - 1u;   // the byte offsets where a token starts
    uint32_t rnd = 0;
    while (alive & (alive - 1)) {
        const uint32_t last = 1u << (31 - __clz(alive));
        uint32_t cand = 0, best = kNoRank;   // cand: ranked and not dropped this round
        for (uint32_t m = alive & ~last; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            const uint32_t r = rk[j * kDropBlock];
            if (r == kNoRank || (A.thr && dropped(wk, rnd, j, A.thr))) continue;
            cand |= 1u << j;
            best = r < best ? r : best;
        }
        if (best == kNoRank) break;
        uint32_t changed = 0;
        for (uint32_t m = alive; m & (m - 1);) {   // left to right; a merged right token is skipped
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            if (((cand >> j) & 1u) && rk[j * kDropBlock] == best) {   // ranks are distinct per pair
                const uint32_t k = (uint32_t)__builtin_ctz(m);
                tk[j * kDropBlock] = pd[j * kDropBlock];
                alive &= ~(1u << k);
                m &= m - 1;
                changed |= 1u << j;
            }
        }
        for (uint32_t m = alive; m & (m - 1);) {   // the pairs beside a merge
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            m &= m - 1;
            const uint32_t k = (uint32_t)__builtin_ctz(m);
            if (((changed >> j) | (changed >> k)) & 1u) {
                const uint2 r = drop_rank(E, tk[j * kDropBlock], tk[k * kDropBlock]);
                rk[j * kDropBlock] = r.x;
                pd[j * kDropBlock] = r.y;
            }
        }
        ++rnd;
    }
    uint32_t cnt = 0;
    for (uint32_t m = alive; m; m &= m - 1) {
        const int64_t v = E.tok2vid[tk[(uint32_t)__builtin_ctz(m) * kDropBlock]];
        if (v < 0) atomicOr(A.status, kDropKey);
        out[cnt++] = (uint32_t)v;
    }
    return cnt;
}

__global__ void __launch_bounds__(kDropBlock) k_drop_merge(DropArgs A, DropTables E) {
    __shared__ uint32_t s_tok[kDropShort * kDropBlock], s_rank[kDropShort * kDropBlock], s_prod[kDropShort * kDropBlock];
    const uint32_t tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
        const uint32_t mc = A.rec_n[c];
        const unsigned long long rb = A.rec_base[c];
        for (uint32_t i0 = 0; i0 < mc; i0 += kDropBlock) {   // (uniform: every lane reaches the append)
            const uint32_t i = i0 + tid;
            bool is_long = false;
            if (i < mc) {
                const uint32_t rec = A.recs[rb + i];
                const RecGeo g = rec_geo(A, c, i, mc, rb);
                uint32_t cnt = 0;
                if (g.end <= g.pos || g.end > A.n) {
                    atomicOr(A.status, kDropBug);
                } else if ((rec & A.kind_mask) == A.kind_special) {   // its one id, no draw
                    const uint32_t k = rec & A.payload_mask;
                    if (k < (uint32_t)E.n_sp) {
                        A.pool[g.pos] = (uint32_t)E.sp_vid[k];
                        cnt = 1;
                    } else {
                        atomicOr(A.status, kDropBug);
                    }
                } else if (g.end - g.pos > (unsigned long long)kDropShort) {
                    is_long = true;
                } else if (g.end - g.pos == 1) {
                    const uint8_t b = A.text[g.pos];
                    if (!(E.n_sp && is_special_word(E, &b, 1))) {
                        const int64_t v = E.tok2vid[E.byte2tok[b]];
                        if (v < 0) atomicOr(A.status, kDropKey);
                        A.pool[g.pos] = (uint32_t)v;
                        cnt = 1;
                    }
                } else {
                    cnt = merge_short(A, E, A.text + g.pos, (uint32_t)(g.end - g.pos), g.wk, s_tok + tid, s_rank + tid,
                                      s_prod + tid, A.pool + g.pos);
                }
                if (!is_long) A.recs[rb + i] = cnt;
            }
            const unsigned at = wave_append(is_long, A.status + 1);
            if (is_long) A.list[at] = ((unsigned long long)c << 16) | i;
        }
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

// One wave per long pre-token.  T (the pool) holds the tokens and ST their byte offsets, dense from
// the pre-token's first byte on; a round reads them 64 at a time and writes the survivors behind
// the read position, so it works in place (a step's loads are complete before its stores: the
// ballot needs them, and the next step reads past everything this one wrote).
__global__ void __launch_bounds__(256) k_drop_long(DropArgs A, DropTables E, unsigned n_long) {
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    const unsigned nwv = gridDim.x * 4;
    for (unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n_long; w += nwv) {
        const unsigned long long ent = A.list[w];
        const size_t c = (size_t)(ent >> 16);
        const uint32_t i = (uint32_t)(ent & 0xffffu);
        const unsigned long long rb = A.rec_base[c];
        const RecGeo g = rec_geo(A, c, i, A.rec_n[c], rb);
        const uint32_t len = (uint32_t)(g.end - g.pos);
        const uint8_t* src = A.text + g.pos;
        uint32_t* T = A.pool + g.pos;
        uint32_t* ST = A.aux + g.pos;
        bool special = false;
        for (int k = 0; k < E.n_sp && !special; ++k) {
            if (E.sp_len[k] != len) continue;
            const uint8_t* sp = E.sp_bytes + E.sp_off[k];
            bool ne = false;
            for (uint32_t j = lane; j < len; j += 64) ne |= src[j] != sp[j];
            special = !__any(ne);
        }
        if (special) {
            if (lane == 0) A.recs[rb + i] = 0;
            continue;
        }
        for (uint32_t j = lane; j < len; j += 64) {
            T[j] = E.byte2tok[src[j]];
            ST[j] = j;
        }
        __threadfence_block();
        uint32_t m = len, rnd = 0;
        while (m > 1) {
            uint32_t best = kNoRank, ba = 0, bb = 0, bp = 0;
            for (uint32_t base = 0; base + 1 < m; base += 64) {
                const uint32_t j = base + lane;
                if (j + 1 < m) {
                    const uint32_t a = T[j], b = T[j + 1];
                    const uint2 r = drop_rank(E, a, b);
                    if (r.x < best && !(A.thr && dropped(g.wk, rnd, ST[j], A.thr))) {
                        best = r.x;
                        ba = a;
                        bb = b;
                        bp = r.y;
                    }
                }
            }
            const uint32_t wbest = wave_min_u32(best);
            if (wbest == kNoRank) break;
            const int leader = __ffsll((long long)__ballot(best == wbest)) - 1;
            ba = __shfl(ba, leader);
            bb = __shfl(bb, leader);
            bp = __shfl(bp, leader);
            uint32_t wpos = 0;
            unsigned long long carry = 0;   // 1: the step's first token was merged into the one before it
            for (uint32_t base = 0; base < m; base += 64) {
                const uint32_t j = base + lane;
                const bool valid = j < m;
                const uint32_t a = valid ? T[j] : 0u, st = valid ? ST[j] : 0u;
                const uint32_t b = j + 1 < m ? T[j + 1] : 0u;
                const bool elig = j + 1 < m && a == ba && b == bb && !(A.thr && dropped(g.wk, rnd, st, A.thr));
                const unsigned long long Em = __ballot(elig);
                unsigned long long Mm = Em;   // the merges: of neighbouring candidates (a pair x, x) every other one
                if ((Em & (Em << 1)) | (Em & carry)) {
                    Mm = 0;
                    unsigned long long prev = carry;
                    for (int q = 0; q < 64; ++q) {
                        const unsigned long long cur = ((Em >> q) & 1ULL) & ~prev;
                        Mm |= cur << q;
                        prev = cur;
                    }
                }
                const unsigned long long Cm = (Mm << 1) | carry;   // merged into their left neighbour
                const unsigned long long Vm = __ballot(valid) & ~Cm;
                if (valid && !((Cm >> lane) & 1ULL)) {
                    const uint32_t idx = wpos + (uint32_t)__popcll(Vm & below);
                    T[idx] = ((Mm >> lane) & 1ULL) ? bp : a;
                    ST[idx] = st;
                }
                wpos += (uint32_t)__popcll(Vm);
                carry = Mm >> 63;
            }
            m = wpos;
            ++rnd;
            __threadfence_block();
        }
        bool bad = false;
        for (uint32_t j = lane; j < m; j += 64) {
            const int64_t v = E.tok2vid[T[j]];
            bad |= v < 0;
            T[j] = (uint32_t)v;
        }
        if (bad) atomicOr(A.status, kDropKey);
        if (lane == 0) A.recs[rb + i] = m;
    }
}

// exclusive scan of v over the 256 threads: this thread's offset; *total = the sum
__device__ __forceinline__ uint32_t drop_block_scan(uint32_t v, uint32_t* s_ws, uint32_t* total) {
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

__global__ void __launch_bounds__(256) k_drop_count(DropArgs A) {
    __shared__ uint32_t s_ws[4];
    for (size_t c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
        const uint32_t mc = A.rec_n[c];
        const uint32_t* r = A.recs + A.rec_base[c];
        uint32_t sum = 0;
        for (uint32_t i = threadIdx.x; i < mc; i += 256) sum += r[i];
        uint32_t total;
        (void)drop_block_scan(sum, s_ws, &total);
        if (threadIdx.x == 0) A.ctot[c] = total;
    }
}

// per chunk, rounds of 256 records: each thread copies its record's ids from the pool to their
// place in the output, and the cuts whose record lies in the round take their id offset
__global__ void __launch_bounds__(256) k_drop_gather(DropArgs A) {
    __shared__ uint32_t s_ws[4];
    __shared__ uint32_t s_pre[256];
    const uint32_t tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
        const uint32_t mc = A.rec_n[c];
        const unsigned long long rb = A.rec_base[c];
        const unsigned long long cbase = (unsigned long long)c * A.chunk;
        const unsigned long long P = A.coff[c];
        uint32_t q = A.chunk_cut0[c];
        const uint32_t q1 = A.chunk_cut0[c + 1];
        uint32_t run = 0;
        for (uint32_t b = 0; b < mc; b += 256) {
            const uint32_t i = b + tid;
            const uint32_t cnt = i < mc ? A.recs[rb + i] : 0u;
            uint32_t total;
            const uint32_t off = drop_block_scan(cnt, s_ws, &total);
            if (cnt) {
                const uint32_t* src = A.pool + cbase + A.rec_pos[rb + i];
                uint32_t* dst = A.out + P + run + off;
                for (uint32_t j = 0; j < cnt; ++j) dst[j] = src[j];
            }
            s_pre[tid] = run + off;
            __syncthreads();
            uint32_t lo = q, hi = q1;   // the first cut whose record is past this round
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (A.cut_rec[mid] < b + 256) lo = mid + 1;
                else hi = mid;
            }
            for (uint32_t k = q + tid; k < lo; k += 256) {
                const uint32_t at = A.cut_rec[k] - b;
                A.cut_off[k] = P + s_pre[at < 256u ? at : 255u];
            }
            q = lo;
            run += total;
            __syncthreads();   // s_pre is reused by the next round
        }
    }
}

constexpr uint32_t kDocAtZero = 0xFFFFFFFFu, kDocAtEnd = 0xFFFFFFFEu;
__global__ void k_drop_doc_offsets(const uint32_t* __restrict__ doc_cut, size_t nd, const unsigned long long* __restrict__ cut_off,
                                   const unsigned long long* __restrict__ coff, const unsigned long long* __restrict__ ctot,
                                   size_t n_chunks, unsigned long long* __restrict__ out) {
    const unsigned long long total = coff[n_chunks - 1] + ctot[n_chunks - 1];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = doc_cut[i];
        out[i] = k == kDocAtZero ? 0ULL : k == kDocAtEnd ? total : cut_off[k];
    }
}

template <class F>
int guarded(F&& f) {
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

void check_params(uint32_t thr, uint64_t doc_base, size_t n_docs) {
    BPE_REQUIRE(thr <= kDropFull, BPE_E_ARG, "thr must be at most 2^24");
    BPE_REQUIRE(doc_base <= UINT64_MAX - (uint64_t)n_docs, BPE_E_ARG, "doc_base + n_docs does not fit 64 bits");
}

}  // namespace

size_t dropout_emit(const DropFront& F, const DropTables& E, const DropParams& P, DropScratch& S, hipStream_t s) {
    const std::vector<unsigned long long>& cuts = *F.h_cuts;
    const size_t nc = cuts.size(), nd = F.n_docs + 1;
    // every cut's document (of several that start there the last: the others are empty), and every
    // document's cut
    std::vector<unsigned long long> cut_doc(std::max<size_t>(nc, 1), 0ULL);
    std::vector<uint32_t> doc_cut(nd);
    unsigned long long doc0 = 0;
    size_t k = 0;
    for (size_t i = 0; i < F.n_docs; ++i) {
        const unsigned long long st = F.h_doc_starts[i];
        if (st == 0) {
            doc0 = i;
            doc_cut[i] = kDocAtZero;
        } else if (st >= F.n) {
            doc_cut[i] = kDocAtEnd;
        } else {
            while (k < nc && cuts[k] < st) ++k;
            BPE_REQUIRE(k < nc && cuts[k] == st, BPE_E_HIP, "internal error: a document start is not a cut");
            cut_doc[k] = i;
            doc_cut[i] = (uint32_t)k;
        }
    }
    doc_cut[F.n_docs] = kDocAtEnd;
    S.pool.reserve(F.n);
    S.ctot.reserve(F.n_chunks);
    S.coff.reserve(F.n_chunks);
    S.cut_off.reserve(std::max<size_t>(nc, 1));
    S.cut_doc.reserve(std::max<size_t>(nc, 1));
    S.doc_cut.reserve(nd);
    S.list.reserve(F.n / kDropShort + 1);   // a listed pre-token is longer than kDropShort
    S.status.reserve(2);
    to_device(S.cut_doc.p, cut_doc.data(), cut_doc.size() * 8, s);
    to_device(S.doc_cut.p, doc_cut.data(), nd * 4, s);
    BPE_HIP(hipMemsetAsync(S.status.p, 0, 8, s));
    DropArgs A{F.text, (unsigned long long)F.n, F.n_chunks, F.chunk, F.recs, F.kind_mask, F.kind_special, F.payload_mask,
               F.rec_pos, F.rec_base, F.rec_n, F.chunk_next, F.cuts, F.chunk_cut0, F.cut_rec, S.cut_doc.p, doc0, P.thr,
               mix64(P.seed + 0x9E3779B97F4A7C15ULL), P.doc_base, S.pool.p, F.d_ids, S.list.p, S.status.p, S.ctot.p,
               S.coff.p, S.cut_off.p, F.d_ids};
    int dev = 0, n_cu = 0, per_cu = 0;
    BPE_HIP(hipGetDevice(&dev));
    BPE_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    n_cu = std::max(1, n_cu);
    BPE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_drop_merge, kDropBlock, 0));
    const unsigned mgrid = (unsigned)std::min<size_t>(F.n_chunks, (size_t)std::max(1, per_cu) * n_cu);
    hipLaunchKernelGGL(k_drop_merge, dim3(mgrid), dim3(kDropBlock), 0, s, A, E);
    BPE_HIP(hipGetLastError());
    unsigned st[2] = {0, 0};
    to_host(st, S.status.p, 8, s);
    if (st[1]) {
        const unsigned lgrid = std::min<unsigned>(ceil_div(st[1], 4), (unsigned)n_cu * 8u);
        hipLaunchKernelGGL(k_drop_long, dim3(lgrid), dim3(256), 0, s, A, E, st[1]);
        BPE_HIP(hipGetLastError());
    }
    const unsigned cgrid = (unsigned)std::min<size_t>(F.n_chunks, (size_t)n_cu * 8);
    hipLaunchKernelGGL(k_drop_count, dim3(cgrid), dim3(256), 0, s, A);
    BPE_HIP(hipGetLastError());
    exclusive_sum(S.ctot.p, S.coff.p, F.n_chunks, s, &S.tmp);
    hipLaunchKernelGGL(k_drop_gather, dim3(cgrid), dim3(256), 0, s, A);
    BPE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_drop_doc_offsets, dim3(grid_for(nd, 256)), dim3(256), 0, s, S.doc_cut.p, nd, S.cut_off.p,
                       S.coff.p, S.ctot.p, F.n_chunks, F.d_id_offsets);
    BPE_HIP(hipGetLastError());
    unsigned long long last[2] = {0, 0};
    to_host(&last[0], S.coff.p + F.n_chunks - 1, 8, s);
    to_host(&last[1], S.ctot.p + F.n_chunks - 1, 8, s);
    to_host(st, S.status.p, 4, s);
    if (st[0] & kDropKey) throw Error{BPE_E_KEY, "a merged token is not in the vocab"};
    BPE_REQUIRE(!(st[0] & kDropBug), BPE_E_HIP, "internal error: encode records inconsistent (dropout)");
    const size_t total = last[0] + last[1];
    BPE_REQUIRE(total <= F.n, BPE_E_HIP, "encode produced more ids than input bytes");
    BPE_HIP(hipStreamSynchronize(s));
    return total;
}

}  // namespace bpe

extern "C" {

int bpe_tok_encode_dropout_device(bpe_tokenizer* tok, const uint8_t* d_utf8, size_t n, const uint64_t* doc_starts,
                                  size_t n_docs, uint32_t thr, uint64_t seed, uint64_t doc_base, uint32_t* d_ids,
                                  size_t* n_out, uint64_t* d_id_offsets, void* hip_stream) {
    return bpe::guarded([&] {
        BPE_REQUIRE(tok && n_out && d_id_offsets && (n == 0 || (d_utf8 && d_ids)), BPE_E_ARG, "NULL argument");
        bpe::check_params(thr, doc_base, n_docs);
        *n_out = bpe::encode_dropout_device(tok, d_utf8, n, doc_starts, n_docs, bpe::DropParams{thr, seed, doc_base}, d_ids,
                                            reinterpret_cast<unsigned long long*>(d_id_offsets), (hipStream_t)hip_stream);
    });
}

int bpe_tok_encode_dropout(bpe_tokenizer* tok, const uint8_t* utf8, size_t n, const uint64_t* doc_starts, size_t n_docs,
                           uint32_t thr, uint64_t seed, uint64_t doc_base, uint32_t* ids_out, size_t cap, size_t* n_out,
                           uint64_t* id_offsets_out) {
    return bpe::guarded([&] {
        BPE_REQUIRE(tok && n_out && id_offsets_out && (n == 0 || (utf8 && ids_out)), BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(cap >= n, BPE_E_ARG, "ids_out capacity must be >= input bytes");
        bpe::check_params(thr, doc_base, n_docs);
        *n_out = 0;
        hipStream_t s = bpe::tokenizer_stream(tok);
        bpe::DevBuf<uint8_t> d_text(n);
        bpe::DevBuf<uint32_t> d_out(n);
        bpe::DevBuf<unsigned long long> d_off(n_docs + 1);
        if (n) BPE_HIP(hipMemcpyAsync(d_text.p, utf8, n, hipMemcpyHostToDevice, s));
        const size_t m = bpe::encode_dropout_device(tok, d_text.p, n, doc_starts, n_docs, bpe::DropParams{thr, seed, doc_base},
                                                    d_out.p, d_off.p, s);
        if (m) BPE_HIP(hipMemcpyAsync(ids_out, d_out.p, m * 4, hipMemcpyDeviceToHost, s));
        BPE_HIP(hipMemcpyAsync(id_offsets_out, d_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
        BPE_HIP(hipStreamSynchronize(s));
        *n_out = m;
    });
}

}  // extern "C"
