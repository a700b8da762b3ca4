// Tokenizer.decode on the device -- reference
// models/tokenizer/tokenizer.py:155-157:
//     raw_bytes = b"".join([self.vocab[i] for i in ids])      <- here: a gather on the GPU
//     return raw_bytes.decode("utf-8", errors="replace")     <- the caller (CPython's decoder,
//                                                               so the replacement rule is exact)
// self.vocab[i] raises KeyError for an id it lacks: BPE_E_KEY here.
//
// Layout: a dense (offset, length) table over ids 0..max_id (length ~0 = no such id) and one
// byte pool.  Decoding: length lookup -> exclusive scan -> one thread per id copies its bytes.

#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "internal.h"
#include "prims.h"

// The batch decode's device arrays, kept by the decoder from call to call (grow-only) so that a
// caller decoding many small batches allocates nothing; a call that grew them past kKeepBytes
// hands them back when it returns.
struct DecScratch {
    static constexpr size_t kKeepBytes = 64u << 20;
    bpe::DevBuf<unsigned long long> ctl;              // kCtlWords control words (below)
    bpe::DevBuf<unsigned long long> lens, tok_off;    // n + 1 each: token byte lengths, their scan
    bpe::DevBuf<unsigned long long> id_off, byte_off; // n_rows + 1 each
    bpe::DevBuf<unsigned long long> span_len, span_c0;   // padded rows: n_rows + 1, n_rows
    bpe::DevBuf<uint32_t> ids;                        // host ids uploaded / padded rows compacted
    bpe::DevBuf<uint8_t> out, tmp;                    // the bytes (host-output calls), rocPRIM's storage
    size_t bytes() const {
        return lens.bytes() + tok_off.bytes() + id_off.bytes() + byte_off.bytes() + span_len.bytes() +
               span_c0.bytes() + ids.bytes() + out.bytes() + tmp.bytes();
    }
    void trim() {
        if (bytes() <= kKeepBytes) return;
        for (auto* b : {&lens, &tok_off, &id_off, &byte_off, &span_len, &span_c0}) b->release();
        ids.release();
        out.release();
        tmp.release();
    }
};

struct bpe_decoder {
    bpe::DevBuf<unsigned long long> off;
    bpe::DevBuf<uint32_t> len;
    bpe::DevBuf<uint8_t> pool;
    uint64_t n_ids = 0;   // table size (max id + 1)
    hipStream_t stream = nullptr;
    DecScratch batch;          // the batch calls' arrays ...
    std::mutex batch_mutex;    // ... which one call at a time uses
    ~bpe_decoder() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace bpe {
namespace {

constexpr uint32_t kNoId = 0xffffffffu;
constexpr uint64_t kMaxDecodeIds = 1ull << 28;   // dense table bound (vocab ids are dense in practice)

__global__ void k_dec_len(const uint32_t* __restrict__ ids, size_t n, const uint32_t* __restrict__ len,
                          uint64_t n_tab, unsigned long long* __restrict__ out_len,
                          unsigned long long* __restrict__ first_bad) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        const uint32_t l = id < n_tab ? len[id] : kNoId;
        if (l == kNoId) {
            atomicMin(first_bad, (unsigned long long)i);
            out_len[i] = 0;
            continue;
        }
        out_len[i] = l;
    }
}

__global__ void k_dec_gather(const uint32_t* __restrict__ ids, size_t n, const unsigned long long* __restrict__ off,
                             const uint32_t* __restrict__ len, const uint8_t* __restrict__ pool,
                             const unsigned long long* __restrict__ out_off, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        const uint32_t l = len[id];
        const uint8_t* src = pool + off[id];
        uint8_t* dst = out + out_off[i];
        for (uint32_t k = 0; k < l; ++k) dst[k] = src[k];
    }
}

template <class F>
int guarded_dec(F&& f) {
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

// d_ids -> bytes at d_out (capacity cap); returns the byte count (or throws)
size_t decode_device(bpe_decoder& D, const uint32_t* d_ids, size_t n, uint8_t* d_out, size_t cap,
                     size_t* needed, hipStream_t s) {
    *needed = 0;
    if (n == 0) return 0;
    DevBuf<unsigned long long> lens(n), offs(n), bad(1);
    const unsigned long long none = ~0ULL;
    BPE_HIP(hipMemcpyAsync(bad.p, &none, 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_dec_len, dim3(grid_for(n, 256)), dim3(256), 0, s, d_ids, n, D.len.p, D.n_ids, lens.p,
                       bad.p);
    exclusive_sum(lens.p, offs.p, n, s);
    unsigned long long h[3];
    BPE_HIP(hipMemcpyAsync(&h[0], offs.p + n - 1, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipMemcpyAsync(&h[1], lens.p + n - 1, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipMemcpyAsync(&h[2], bad.p, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipStreamSynchronize(s));
    if (h[2] != none) {
        uint32_t id = 0;
        BPE_HIP(hipMemcpy(&id, d_ids + h[2], 4, hipMemcpyDeviceToHost));
        throw Error{BPE_E_KEY, std::to_string(id)};
    }
    const size_t total = (size_t)(h[0] + h[1]);
    *needed = total;
    BPE_REQUIRE(cap >= total, BPE_E_ARG, "decode output capacity too small");
    hipLaunchKernelGGL(k_dec_gather, dim3(grid_for(n, 256)), dim3(256), 0, s, d_ids, n, D.off.p, D.len.p,
                       D.pool.p, offs.p, d_out);
    BPE_HIP(hipGetLastError());
    BPE_HIP(hipStreamSynchronize(s));
    return total;
}

// ------------------------------------------------------------------ batch decode
// Many rows of ids (CSR: flat ids + row offsets, or a padded matrix compacted to that) -> the rows'
// bytes, concatenated, and where each row begins.  One pass, no size query:
//   [padded rows only: k_rows_span -> scan -> k_rows_copy]
//   k_dec_len -> one scan over n + 1 lengths (the last entry is the total) -> k_dec_row_off
//   -> one read-back of the control words -> k_dec_gather_tiled.
// A row boundary costs nothing in the gather: the output is one contiguous byte stream, and row
// i begins at tok_off[id_offsets[i]].
//
// Control words, set to ~0 before a call:
enum : int {
    kCtlBad = 0,     // flat index of the first id without an entry (atomicMin)
    kCtlOk = 1,      // 0: the offsets / lengths were rejected
    kCtlTotal = 2,   // tok_off[n], the byte total
    kCtlValue = 3,   // padded rows: the matrix entry at flat index kCtlBad (k_rows_value)
    kCtlWords = 4
};

// Tile of the gather: kDecTileIds consecutive ids per 256-thread workgroup (8 per thread), their
// bytes assembled in a kDecTileBytes LDS buffer.  16 KiB per workgroup lets the 8 workgroups that
// a CU's 32 wave slots admit stay resident together (128 of the CU's 160 KiB), and holds a tile
// up to 8 bytes per id on average; GPT-2 ids of English text average under 5.
constexpr unsigned kDecTileIds = 2048;
constexpr unsigned kDecTileBytes = 16384;
constexpr unsigned kDecLongToken = 64;  // overflow path: longer tokens are copied by the whole workgroup
static_assert(kDecTileIds * sizeof(unsigned) <= kDecTileBytes, "the overflow path lists ids in the byte buffer");
// DESIGN.md section 4, The batch decode: the measured choice between the tiled and the per-id gather
constexpr bool kBatchTiledGather = true;

constexpr int kRowsKeepStop = 1, kRowsLeftPadded = 2;

// byte_off[i] = tok_off[id_off[i]] for the n_rows + 1 row offsets, which are checked on the way
// (first 0, non-decreasing, last n); the byte total goes to the control words.
__global__ void k_dec_row_off(const unsigned long long* __restrict__ id_off, size_t n_rows, size_t n,
                              const unsigned long long* __restrict__ tok_off,
                              unsigned long long* __restrict__ byte_off, unsigned long long* __restrict__ ctl) {
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) ctl[kCtlTotal] = tok_off[n];
    for (size_t i = t0; i <= n_rows; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long a = id_off[i];
        const bool ok = a <= n && (i > 0 || a == 0) && (i < n_rows ? id_off[i + 1] >= a : a == n);
        if (!ok) ctl[kCtlOk] = 0;
        byte_off[i] = a <= n ? tok_off[a] : 0;
    }
}

// The hot kernel.  A workgroup takes a tile of consecutive ids (rows do not matter: the tile's
// bytes are the contiguous range [tok_off[j0], tok_off[j0 + m]) of the output), copies each token
// from the pool to its place in LDS, and stores the range with 16-byte writes: a scalar head up to
// the destination's 16-byte alignment, the uint4 body, a scalar tail (the shape of k_enc_emit's
// write pass).  The LDS image starts at the destination's misalignment, so the body's LDS reads
// are 16-byte aligned as well.  A token's length is the difference of two neighbouring offsets (a
// coalesced read instead of a second table lookup).  A tile whose bytes do not fit the buffer goes
// straight to memory: tokens up to kDecLongToken bytes by their own thread, longer ones, listed in
// the idle buffer, by all 256 threads together (a vocab may hold arbitrarily long entries).
__global__ void __launch_bounds__(256, 8)   // 8 waves per SIMD: the 8 workgroups per CU the LDS buffer is sized for
k_dec_gather_tiled(const uint32_t* __restrict__ ids, size_t n, const unsigned long long* __restrict__ off,
                   const uint8_t* __restrict__ pool, const unsigned long long* __restrict__ tok_off,
                   uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t buf[kDecTileBytes];
    __shared__ unsigned s_long;
    const unsigned tid = threadIdx.x;
    const size_t n_tiles = (n + kDecTileIds - 1) / kDecTileIds;
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t j0 = t * kDecTileIds;
        const unsigned m = n - j0 < kDecTileIds ? (unsigned)(n - j0) : kDecTileIds;
        const unsigned long long base = tok_off[j0];
        const unsigned long long T = tok_off[j0 + m] - base;
        uint8_t* dst = out + base;
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15);
        if (T + mis <= kDecTileBytes) {
            for (unsigned q = tid; q < m; q += 256) {
                const unsigned long long a = tok_off[j0 + q];
                const unsigned l = (unsigned)(tok_off[j0 + q + 1] - a);
                const uint8_t* src = pool + off[ids[j0 + q]];
                uint8_t* d = buf + mis + (unsigned)(a - base);
                for (unsigned k = 0; k < l; ++k) d[k] = src[k];
            }
            __syncthreads();
            const unsigned Tn = (unsigned)T;
            const unsigned head = (16 - mis) & 15;
            const unsigned h = head < Tn ? head : Tn;
            if (tid < h) dst[tid] = buf[mis + tid];
            const unsigned body = (Tn - h) / 16;   // h < head: Tn == h, no body
            const uint4* sb = reinterpret_cast<const uint4*>(buf + mis + h);
            uint4* db = reinterpret_cast<uint4*>(dst + h);
            for (unsigned i = tid; i < body; i += 256) db[i] = sb[i];
            for (unsigned q = h + 16 * body + tid; q < Tn; q += 256) dst[q] = buf[mis + q];
            __syncthreads();   // buf is reused by the next tile
        } else {
            unsigned* list = reinterpret_cast<unsigned*>(buf);
            if (tid == 0) s_long = 0;
            __syncthreads();
            for (unsigned q = tid; q < m; q += 256) {
                const unsigned long long a = tok_off[j0 + q];
                const unsigned long long l = tok_off[j0 + q + 1] - a;
                if (l > kDecLongToken) {
                    list[atomicAdd(&s_long, 1u)] = q;
                    continue;
                }
                const uint8_t* src = pool + off[ids[j0 + q]];
                uint8_t* d = out + a;
                for (unsigned k = 0; k < (unsigned)l; ++k) d[k] = src[k];
            }
            __syncthreads();
            const unsigned n_long = s_long;
            for (unsigned e = 0; e < n_long; ++e) {
                const unsigned q = list[e];
                const unsigned long long a = tok_off[j0 + q];
                const unsigned long long l = tok_off[j0 + q + 1] - a;
                const uint8_t* src = pool + off[ids[j0 + q]];
                uint8_t* d = out + a;
                for (unsigned long long k = tid; k < l; k += 256) d[k] = src[k];
            }
            __syncthreads();   // list and s_long are reused by the next tile
        }
    }
}

// Padded rows, first pass: the kept span of every row (bpe355.h, bpe_dec_decode_rows_device), one
// wave per row.  The span is [c0, c0 + L) of the row: the lengths[i] first entries, or with
// kRowsLeftPadded the last; all of the row without lengths; cut at the first entry equal to
// stop_id (kRowsKeepStop: behind it), found 64 entries at a time.  Nothing outside the span is read.
template <class T>
__global__ void __launch_bounds__(256)
k_rows_span(const T* __restrict__ rows, size_t n_rows, size_t row_len, const int32_t* __restrict__ lengths,
            long long stop_id, int flags, unsigned long long* __restrict__ span_len,
            unsigned long long* __restrict__ span_c0, unsigned long long* __restrict__ ctl) {
    const unsigned lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    if (wave == 0 && lane == 0) span_len[n_rows] = 0;   // the scan's last entry: the id total
    for (size_t i = wave; i < n_rows; i += n_waves) {
        unsigned long long L = row_len;
        if (lengths) {
            const long long v = lengths[i];
            if (v < 0 || (unsigned long long)v > row_len) {
                if (lane == 0) ctl[kCtlOk] = 0;
                L = 0;
            } else {
                L = (unsigned long long)v;
            }
        }
        const unsigned long long c0 = (flags & kRowsLeftPadded) ? row_len - L : 0;
        if (stop_id >= 0) {
            const T* r = rows + i * row_len + c0;
            for (unsigned long long b = 0; b < L; b += 64) {   // L and b are the same in every lane
                const bool hit = b + lane < L && (long long)r[b + lane] == stop_id;
                const unsigned long long mask = __ballot(hit);
                if (mask) {
                    L = b + (unsigned)(__ffsll((long long)mask) - 1) + ((flags & kRowsKeepStop) ? 1 : 0);
                    break;
                }
            }
        }
        if (lane == 0) {
            span_len[i] = L;
            span_c0[i] = c0;
        }
    }
}

// Second pass: the kept entries -> uint32 CSR ids at id_off[i] (the scan of the span lengths).  An
// entry outside [0, 2^32) has no id: its flat index goes to the control word k_dec_len uses for an
// id without a vocab entry, so the first of either kind is the one reported.
template <class T>
__global__ void __launch_bounds__(256)
k_rows_copy(const T* __restrict__ rows, size_t n_rows, size_t row_len, const unsigned long long* __restrict__ span_len,
            const unsigned long long* __restrict__ span_c0, const unsigned long long* __restrict__ id_off,
            uint32_t* __restrict__ ids, unsigned long long* __restrict__ ctl) {
    const unsigned lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t i = wave; i < n_rows; i += n_waves) {
        const unsigned long long L = span_len[i], a = id_off[i];
        const T* r = rows + i * row_len + span_c0[i];
        for (unsigned long long c = lane; c < L; c += 64) {
            const long long v = (long long)r[c];
            if (v < 0 || v > 0xffffffffLL) atomicMin(&ctl[kCtlBad], a + c);
            ids[a + c] = (uint32_t)v;
        }
    }
}

// Error path of the padded rows: the matrix entry behind flat id index f, as the caller wrote it
template <class T>
__global__ void k_rows_value(const T* __restrict__ rows, size_t n_rows, size_t row_len,
                             const unsigned long long* __restrict__ span_c0,
                             const unsigned long long* __restrict__ id_off, unsigned long long f,
                             unsigned long long* __restrict__ ctl) {
    size_t lo = 0, hi = n_rows;   // id_off[lo] <= f < id_off[hi]
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (id_off[mid] <= f) lo = mid; else hi = mid;
    }
    ctl[kCtlValue] = (unsigned long long)(long long)rows[lo * row_len + span_c0[lo] + (f - id_off[lo])];
}

struct TrimOnExit {
    DecScratch& s;
    ~TrimOnExit() { s.trim(); }
};

void ctl_init(DecScratch& S, hipStream_t s) {
    S.ctl.reserve(kCtlWords);
    BPE_HIP(hipMemsetAsync(S.ctl.p, 0xff, kCtlWords * 8, s));
}

// Token lengths, their scan into tok_off (n + 1), the rows' byte offsets (n_rows + 1) and the one
// read-back of a call: returns the byte total, or throws BPE_E_ARG for bad offsets / BPE_E_KEY with
// key_msg(flat index) for an id without an entry.  The control words were initialised by the caller.
template <class KeyMsg>
size_t batch_offsets(bpe_decoder& D, const uint32_t* d_ids, size_t n, const unsigned long long* d_id_off,
                     size_t n_rows, unsigned long long* tok_off, unsigned long long* d_byte_off, hipStream_t s,
                     KeyMsg&& key_msg) {
    DecScratch& S = D.batch;
    S.lens.reserve(n + 1);
    if (n)
        hipLaunchKernelGGL(k_dec_len, dim3(grid_for(n, 256)), dim3(256), 0, s, d_ids, n, D.len.p, D.n_ids, S.lens.p,
                           S.ctl.p + kCtlBad);
    BPE_HIP(hipMemsetAsync(S.lens.p + n, 0, 8, s));
    exclusive_sum(S.lens.p, tok_off, n + 1, s, &S.tmp);
    hipLaunchKernelGGL(k_dec_row_off, dim3(grid_for(n_rows + 1, 256)), dim3(256), 0, s, d_id_off, n_rows, n, tok_off,
                       d_byte_off, S.ctl.p);
    BPE_HIP(hipGetLastError());
    unsigned long long h[3];
    BPE_HIP(hipMemcpyAsync(h, S.ctl.p, sizeof(h), hipMemcpyDeviceToHost, s));
    BPE_HIP(hipStreamSynchronize(s));
    BPE_REQUIRE(h[kCtlOk] != 0, BPE_E_ARG, "id_offsets must start at 0, not decrease and end at n");
    if (h[kCtlBad] != ~0ULL) throw Error{BPE_E_KEY, key_msg((size_t)h[kCtlBad])};
    return (size_t)h[kCtlTotal];
}

void batch_gather(bpe_decoder& D, const uint32_t* d_ids, size_t n, const unsigned long long* tok_off,
                  uint8_t* d_out, size_t total, hipStream_t s) {
    if (!total) return;
    if (kBatchTiledGather) {
        const size_t tiles = (n + kDecTileIds - 1) / kDecTileIds;
        const unsigned grid = (unsigned)std::min<size_t>(tiles, 2048);   // 8 workgroups on each of 256 CUs
        hipLaunchKernelGGL(k_dec_gather_tiled, dim3(grid), dim3(256), 0, s, d_ids, n, D.off.p, D.pool.p, tok_off,
                           d_out);
    } else {
        hipLaunchKernelGGL(k_dec_gather, dim3(grid_for(n, 256)), dim3(256), 0, s, d_ids, n, D.off.p, D.len.p,
                           D.pool.p, tok_off, d_out);
    }
    BPE_HIP(hipGetLastError());
}

// The host-output calls' second half: gather into the scratch buffer, one copy back of the bytes
// and the offsets, one synchronisation.
void batch_to_host(bpe_decoder& D, const uint32_t* d_ids, size_t n, size_t n_rows, const unsigned long long* tok_off,
                   size_t total, uint8_t** bytes_out, size_t* n_bytes, uint64_t* byte_offsets_out,
                   uint64_t* token_offsets_out, hipStream_t s) {
    DecScratch& S = D.batch;
    S.out.reserve(std::max<size_t>(total, 1));
    batch_gather(D, d_ids, n, tok_off, S.out.p, total, s);
    std::unique_ptr<uint8_t, void (*)(void*)> h((uint8_t*)std::malloc(std::max<size_t>(total, 1)), std::free);
    if (!h) throw std::bad_alloc();
    if (total) BPE_HIP(hipMemcpyAsync(h.get(), S.out.p, total, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipMemcpyAsync(byte_offsets_out, S.byte_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
    if (token_offsets_out)
        BPE_HIP(hipMemcpyAsync(token_offsets_out, tok_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipStreamSynchronize(s));
    *bytes_out = h.release();
    *n_bytes = total;
}

template <class T>
void decode_rows(bpe_decoder& D, const T* d_rows, size_t n_rows, size_t row_len, const int32_t* d_lengths,
                 int64_t stop_id, int flags, uint8_t** bytes_out, size_t* n_bytes, uint64_t* byte_offsets_out,
                 hipStream_t s) {
    DecScratch& S = D.batch;
    ctl_init(S, s);
    S.span_len.reserve(n_rows + 1);
    S.span_c0.reserve(std::max<size_t>(n_rows, 1));
    S.id_off.reserve(n_rows + 1);
    S.byte_off.reserve(n_rows + 1);
    const unsigned grid = grid_for(std::max<size_t>(n_rows, 1), 4);   // a wave per row, 4 rows per workgroup
    hipLaunchKernelGGL(k_rows_span<T>, dim3(grid), dim3(256), 0, s, d_rows, n_rows, row_len, d_lengths,
                       (long long)stop_id, flags, S.span_len.p, S.span_c0.p, S.ctl.p);
    exclusive_sum(S.span_len.p, S.id_off.p, n_rows + 1, s, &S.tmp);
    BPE_HIP(hipGetLastError());
    unsigned long long n64 = 0, ok = 0;   // the id total sizes the next arrays: one synchronisation more
    BPE_HIP(hipMemcpyAsync(&n64, S.id_off.p + n_rows, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipMemcpyAsync(&ok, S.ctl.p + kCtlOk, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipStreamSynchronize(s));
    BPE_REQUIRE(ok != 0, BPE_E_ARG, "a row length is outside [0, row_len]");
    const size_t n = (size_t)n64;
    S.ids.reserve(std::max<size_t>(n, 1));
    S.tok_off.reserve(n + 1);
    if (n)
        hipLaunchKernelGGL(k_rows_copy<T>, dim3(grid), dim3(256), 0, s, d_rows, n_rows, row_len, S.span_len.p,
                           S.span_c0.p, S.id_off.p, S.ids.p, S.ctl.p);
    const size_t total = batch_offsets(D, S.ids.p, n, S.id_off.p, n_rows, S.tok_off.p, S.byte_off.p, s, [&](size_t f) {
        hipLaunchKernelGGL(k_rows_value<T>, dim3(1), dim3(1), 0, s, d_rows, n_rows, row_len, S.span_c0.p, S.id_off.p,
                           (unsigned long long)f, S.ctl.p);
        long long v = 0;
        BPE_HIP(hipMemcpyAsync(&v, S.ctl.p + kCtlValue, 8, hipMemcpyDeviceToHost, s));
        BPE_HIP(hipStreamSynchronize(s));
        return std::to_string(v);
    });
    batch_to_host(D, S.ids.p, n, n_rows, S.tok_off.p, total, bytes_out, n_bytes, byte_offsets_out, nullptr, s);
}

}  // namespace
}  // namespace bpe

extern "C" {

int bpe_dec_create(const uint8_t* vocab_blob, size_t vocab_n, bpe_decoder** out) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(out && (vocab_n == 0 || vocab_blob), BPE_E_ARG, "NULL argument");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw bpe::Error{BPE_E_HIP, "no HIP device visible (libbpe355 needs an MI355X / gfx950 GPU)"};
        // blob: u32 count, then (i64 id, u32 len, bytes) per entry
        const uint8_t* p = vocab_blob;
        const uint8_t* end = vocab_blob + vocab_n;
        BPE_REQUIRE(vocab_n >= 4, BPE_E_ARG, "truncated vocab blob");
        uint32_t nv;
        std::memcpy(&nv, p, 4);
        p += 4;
        std::vector<std::pair<uint64_t, std::string>> ents;
        uint64_t max_id = 0;
        for (uint32_t i = 0; i < nv; ++i) {
            BPE_REQUIRE(p + 12 <= end, BPE_E_ARG, "truncated vocab blob");
            int64_t id;
            uint32_t l;
            std::memcpy(&id, p, 8);
            std::memcpy(&l, p + 8, 4);
            p += 12;
            BPE_REQUIRE(p + l <= end, BPE_E_ARG, "truncated vocab blob");
            BPE_REQUIRE(id >= 0 && (uint64_t)id < bpe::kMaxDecodeIds, BPE_E_LIMIT, "vocab id outside [0, 2^28)");
            ents.emplace_back((uint64_t)id, std::string((const char*)p, l));
            max_id = std::max<uint64_t>(max_id, (uint64_t)id);
            p += l;
        }
        auto D = std::make_unique<bpe_decoder>();
        D->n_ids = ents.empty() ? 0 : max_id + 1;
        std::vector<unsigned long long> off(std::max<uint64_t>(D->n_ids, 1), 0);
        std::vector<uint32_t> len(std::max<uint64_t>(D->n_ids, 1), bpe::kNoId);
        std::string pool;
        for (const auto& e : ents) {   // a repeated id: the later entry wins, as in a dict literal
            off[e.first] = pool.size();
            len[e.first] = (uint32_t)e.second.size();
            pool += e.second;
        }
        BPE_HIP(hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking));
        D->off.alloc(off.size());
        D->len.alloc(len.size());
        D->pool.alloc(std::max<size_t>(pool.size(), 1));
        BPE_HIP(hipMemcpyAsync(D->off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, D->stream));
        BPE_HIP(hipMemcpyAsync(D->len.p, len.data(), len.size() * 4, hipMemcpyHostToDevice, D->stream));
        if (!pool.empty())
            BPE_HIP(hipMemcpyAsync(D->pool.p, pool.data(), pool.size(), hipMemcpyHostToDevice, D->stream));
        BPE_HIP(hipStreamSynchronize(D->stream));
        *out = D.release();
    });
}

int bpe_dec_decode(bpe_decoder* dec, const uint32_t* ids, size_t n, uint8_t* out, size_t cap, size_t* n_out) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(dec && n_out && (n == 0 || ids), BPE_E_ARG, "NULL argument");
        *n_out = 0;
        if (n == 0) return;
        bpe::DevBuf<uint32_t> d_ids(n);
        BPE_HIP(hipMemcpyAsync(d_ids.p, ids, n * 4, hipMemcpyHostToDevice, dec->stream));
        // size first, then gather into a device buffer of exactly that size
        size_t needed = 0;
        try {
            bpe::decode_device(*dec, d_ids.p, n, nullptr, 0, &needed, dec->stream);
        } catch (const bpe::Error& e) {
            if (e.code != BPE_E_ARG) throw;
        }
        *n_out = needed;
        BPE_REQUIRE(out || needed == 0, BPE_E_ARG, "NULL output");
        BPE_REQUIRE(cap >= needed, BPE_E_ARG, "decode output capacity too small");
        bpe::DevBuf<uint8_t> d_out(std::max<size_t>(needed, 1));
        const size_t m = bpe::decode_device(*dec, d_ids.p, n, d_out.p, needed, &needed, dec->stream);
        if (m) BPE_HIP(hipMemcpyAsync(out, d_out.p, m, hipMemcpyDeviceToHost, dec->stream));
        BPE_HIP(hipStreamSynchronize(dec->stream));
    });
}

int bpe_dec_decode_device(bpe_decoder* dec, const uint32_t* d_ids, size_t n, uint8_t* d_out, size_t cap,
                          size_t* n_out, void* hip_stream) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(dec && n_out && (n == 0 || d_ids), BPE_E_ARG, "NULL argument");
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : dec->stream;
        size_t needed = 0;
        *n_out = 0;
        try {
            *n_out = bpe::decode_device(*dec, d_ids, n, d_out, cap, &needed, s);
        } catch (const bpe::Error& e) {
            if (e.code == BPE_E_ARG) *n_out = needed;   // capacity too small: report the size
            throw;
        }
    });
}

int bpe_dec_decode_batch(bpe_decoder* dec, const uint32_t* ids, size_t n, const uint64_t* id_offsets,
                         size_t n_rows, uint8_t** bytes_out, size_t* n_bytes, uint64_t* byte_offsets_out,
                         uint64_t* token_offsets_out) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(dec && id_offsets && bytes_out && n_bytes && byte_offsets_out && (n == 0 || ids), BPE_E_ARG,
                    "NULL argument");
        *bytes_out = nullptr;
        *n_bytes = 0;
        bool ok = id_offsets[0] == 0 && id_offsets[n_rows] == n;
        for (size_t i = 0; ok && i < n_rows; ++i) ok = id_offsets[i] <= id_offsets[i + 1];
        BPE_REQUIRE(ok, BPE_E_ARG, "id_offsets must start at 0, not decrease and end at n");
        std::lock_guard<std::mutex> lock(dec->batch_mutex);
        DecScratch& S = dec->batch;
        bpe::TrimOnExit trim{S};
        hipStream_t s = dec->stream;
        bpe::ctl_init(S, s);
        S.ids.reserve(std::max<size_t>(n, 1));
        S.id_off.reserve(n_rows + 1);
        S.byte_off.reserve(n_rows + 1);
        S.tok_off.reserve(n + 1);
        if (n) BPE_HIP(hipMemcpyAsync(S.ids.p, ids, n * 4, hipMemcpyHostToDevice, s));
        BPE_HIP(hipMemcpyAsync(S.id_off.p, id_offsets, (n_rows + 1) * 8, hipMemcpyHostToDevice, s));
        const size_t total = bpe::batch_offsets(*dec, S.ids.p, n, S.id_off.p, n_rows, S.tok_off.p, S.byte_off.p, s,
                                                [&](size_t f) { return std::to_string(ids[f]); });
        bpe::batch_to_host(*dec, S.ids.p, n, n_rows, S.tok_off.p, total, bytes_out, n_bytes, byte_offsets_out,
                           token_offsets_out, s);
    });
}

int bpe_dec_decode_batch_device(bpe_decoder* dec, const uint32_t* d_ids, size_t n, const uint64_t* d_id_offsets,
                                size_t n_rows, uint8_t* d_out, size_t cap, size_t* n_out, uint64_t* d_byte_offsets,
                                uint64_t* d_token_offsets, void* hip_stream) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(dec && n_out && d_id_offsets && d_byte_offsets && (n == 0 || d_ids), BPE_E_ARG, "NULL argument");
        *n_out = 0;
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : dec->stream;
        std::lock_guard<std::mutex> lock(dec->batch_mutex);
        DecScratch& S = dec->batch;
        bpe::TrimOnExit trim{S};
        bpe::ctl_init(S, s);
        unsigned long long* tok_off = reinterpret_cast<unsigned long long*>(d_token_offsets);
        if (!tok_off) {
            S.tok_off.reserve(n + 1);
            tok_off = S.tok_off.p;
        }
        const size_t total = bpe::batch_offsets(
            *dec, d_ids, n, reinterpret_cast<const unsigned long long*>(d_id_offsets), n_rows, tok_off,
            reinterpret_cast<unsigned long long*>(d_byte_offsets), s, [&](size_t f) {
                uint32_t id = 0;
                BPE_HIP(hipMemcpy(&id, d_ids + f, 4, hipMemcpyDeviceToHost));
                return std::to_string(id);
            });
        *n_out = total;   // also when cap is too small: the size to come back with
        BPE_REQUIRE(cap >= total, BPE_E_ARG, "decode output capacity too small");
        BPE_REQUIRE(d_out || total == 0, BPE_E_ARG, "NULL output");
        bpe::batch_gather(*dec, d_ids, n, tok_off, d_out, total, s);
        BPE_HIP(hipStreamSynchronize(s));
    });
}

int bpe_dec_decode_rows_device(bpe_decoder* dec, const void* d_rows, int elem_bytes, size_t n_rows, size_t row_len,
                               const int32_t* d_lengths, int64_t stop_id, int flags, uint8_t** bytes_out,
                               size_t* n_bytes, uint64_t* byte_offsets_out, void* hip_stream) {
    return bpe::guarded_dec([&] {
        BPE_REQUIRE(dec && bytes_out && n_bytes && byte_offsets_out, BPE_E_ARG, "NULL argument");
        *bytes_out = nullptr;
        *n_bytes = 0;
        BPE_REQUIRE(elem_bytes == 4 || elem_bytes == 8, BPE_E_ARG, "elem_bytes must be 4 or 8");
        BPE_REQUIRE((flags & ~(bpe::kRowsKeepStop | bpe::kRowsLeftPadded)) == 0, BPE_E_ARG, "unknown flags");
        BPE_REQUIRE(row_len <= (size_t)INT32_MAX, BPE_E_ARG, "row_len does not fit the int32 lengths");
        BPE_REQUIRE(row_len == 0 || n_rows <= SIZE_MAX / 8 / row_len, BPE_E_ARG, "n_rows x row_len overflows");
        BPE_REQUIRE(d_rows || n_rows == 0 || row_len == 0, BPE_E_ARG, "NULL argument");
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : dec->stream;
        std::lock_guard<std::mutex> lock(dec->batch_mutex);
        bpe::TrimOnExit trim{dec->batch};
        if (elem_bytes == 4)
            bpe::decode_rows(*dec, static_cast<const int32_t*>(d_rows), n_rows, row_len, d_lengths, stop_id, flags,
                             bytes_out, n_bytes, byte_offsets_out, s);
        else
            bpe::decode_rows(*dec, static_cast<const int64_t*>(d_rows), n_rows, row_len, d_lengths, stop_id, flags,
                             bytes_out, n_bytes, byte_offsets_out, s);
    });
}

void bpe_dec_free(bpe_decoder* dec) { delete dec; }

}  // extern "C"
