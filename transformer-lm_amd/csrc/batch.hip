// The batch loader: windows of a token stream -> the [B, T] input and target matrices a training
// step consumes (the reference's load_batch, models/util.py:37-57, which slices a memmap row by
// row in Python), and, from the separator index the dataset encoder writes, each token's position
// inside its document and the row's segment ids.
//
//   k_batch_rows        : one workgroup per tile of kBatchTile outputs of one row
//   bpe_batch_stage_*   : the same for a stream that lives in host memory (two pinned and two
//                         device buffers, handed over by events)
//
// A tile reads its ids once, as 16-byte vectors on the 16-byte grid of the address space
// (load_ids: the stream is aligned to its element size only and a row starts at any element), into
// LDS; inputs and targets are both written from that copy, as 16-byte stores from the first
// 16-byte boundary of the tile's output on and element stores before it and after the last whole
// vector.
//
// The document outputs are functions of the global index alone: positions = g - (the largest
// separator position < g, or -1) - 1, doc_ids = the separators in [row start, g).  A tile finds the
// last separator before its first index and the separators before the row with binary searches of
// the sorted index, marks the index entries that fall inside it in LDS, and finishes with a
// max-scan and a count over its own elements.  No tile waits for another one.
#include <algorithm>
#include <climits>
#include <cstring>
#include <thread>
#include <vector>

#include "idload.h"
#include "internal.h"

namespace bpe {
namespace {

constexpr unsigned kBatchTile = 1024;      // outputs of one row per workgroup step: 4 per thread
constexpr unsigned kBatchThreads = 256;
constexpr unsigned kPerThread = kBatchTile / kBatchThreads;
// the status word: ~0 = nothing to report; below kLimitBit the smallest row that was out of range;
// else kLimitBit | the smallest id that does not fit int32 (a bad row wins over an id: atomicMin)
constexpr unsigned long long kLimitBit = 1ull << 62;

struct BatchParams {
    const void* ids;
    size_t n;
    unsigned sh;                    // elements of grid vector 0 that lie before ids[0]
    const long long* src;
    const long long* pos;           // NULL: src
    size_t n_rows;
    unsigned row_len;
    void* inputs;
    void* targets;
    long long* positions;
    int* doc_ids;
    const unsigned long long* sep;
    size_t n_sep;
    unsigned sep_id;
    int ignore;                     // targets = ignore_index where inputs == sep_id
    long long ignore_index;
    unsigned long long* status;
};

// how many of sep[0, n) are below x
__device__ __forceinline__ size_t lower_bound_u64(const unsigned long long* __restrict__ sep, size_t n,
                                                  unsigned long long x) {
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (sep[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// exclusive block scan of (max, sum) over the threads in order; wmx/wc: 4 LDS words each
__device__ __forceinline__ void block_excl_max_sum(int& mx, unsigned& c, int* wmx, unsigned* wc) {
    const unsigned lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int imx = mx;
    unsigned ic = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int tm = __shfl_up(imx, o);
        const unsigned tc = __shfl_up(ic, o);
        if ((int)lane >= o) {
            imx = tm > imx ? tm : imx;
            ic += tc;
        }
    }
    if (lane == 63) {
        wmx[w] = imx;
        wc[w] = ic;
    }
    int emx = __shfl_up(imx, 1);
    unsigned ec = __shfl_up(ic, 1);
    if (lane == 0) {
        emx = -1;
        ec = 0;
    }
    __syncthreads();
#pragma unroll
    for (unsigned i = 0; i < kBatchThreads / 64; ++i)
        if (i < w) {
            emx = wmx[i] > emx ? wmx[i] : emx;
            ec += wc[i];
        }
    mx = emx;
    c = ec;
}

// out[0, len) = val(e): element stores up to the first 16-byte boundary and after the last whole
// vector, 16-byte stores between them
template <class O, class F>
__device__ __forceinline__ void store_tile(O* __restrict__ out, unsigned len, F&& val) {
    constexpr unsigned VO = 16 / sizeof(O);
    const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(out) & 15u) / sizeof(O));
    const unsigned head = min(len, (VO - mis) % VO);
    const unsigned nvec = (len - head) / VO;
    const unsigned tail0 = head + nvec * VO;
    if (threadIdx.x < head) out[threadIdx.x] = val(threadIdx.x);
    if (tail0 + threadIdx.x < len) out[tail0 + threadIdx.x] = val(tail0 + threadIdx.x);
    for (unsigned i = threadIdx.x; i < nvec; i += kBatchThreads) {
        const unsigned e = head + i * VO;
        union { uint4 w; O o[VO]; } u;
#pragma unroll
        for (unsigned k = 0; k < VO; ++k) u.o[k] = val(e + k);
        *reinterpret_cast<uint4*>(out + e) = u.w;
    }
}

template <class O>
__device__ __forceinline__ O id_out(unsigned id, unsigned long long* status) {
    if (sizeof(O) == 4 && id >= 0x80000000u && status) atomicMin(status, kLimitBit | (unsigned long long)id);
    return (O)id;
}

template <class E, class O>
__global__ void __launch_bounds__(kBatchThreads) k_batch_rows(const BatchParams p) {
    constexpr unsigned V = 16 / sizeof(E);
    __shared__ unsigned s_id[kBatchTile + 1];
    __shared__ long long s_posn[kBatchTile];
    __shared__ int s_doc[kBatchTile];
    __shared__ unsigned char s_flag[kBatchTile];
    __shared__ unsigned long long s_k[3];
    __shared__ int s_wmx[kBatchThreads / 64];
    __shared__ unsigned s_wc[kBatchThreads / 64];
    const E* __restrict__ ids = static_cast<const E*>(p.ids);
    const unsigned tid = threadIdx.x;
    const unsigned extra = p.targets ? 1u : 0u;
    const size_t tiles_per_row = ((size_t)p.row_len + kBatchTile - 1) / kBatchTile;
    const size_t n_tiles = p.n_rows * tiles_per_row;
    // the last source offset whose row lies inside [0, n)
    const long long limit = (long long)p.n - (long long)p.row_len - (long long)extra;
    const bool docs = p.positions || p.doc_ids;

    for (size_t ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
        const size_t r = ti / tiles_per_row;
        const unsigned t0 = (unsigned)(ti % tiles_per_row) * kBatchTile;
        const unsigned len = min(kBatchTile, p.row_len - t0);
        const long long s = p.src[r];
        if (s < 0 || s > limit) {   // uniform over the workgroup: the row is neither read nor written
            if (tid == 0 && t0 == 0 && p.status) atomicMin(p.status, (unsigned long long)r);
            continue;
        }
        __syncthreads();   // the previous tile's LDS has been read

        // ---- the tile's ids, read once
        const size_t first = (size_t)s + t0;
        const unsigned need = len + extra;
        const size_t j0 = (first + p.sh) / V, j1 = (first + need - 1 + p.sh) / V;
        for (size_t j = j0 + tid; j <= j1; j += kBatchThreads) {
            E v[V];
            const unsigned m = load_ids(ids, p.n, p.sh, j, v);
            const long long rel0 = (long long)(j * V) - (long long)p.sh - (long long)first;
#pragma unroll
            for (unsigned k = 0; k < V; ++k) {
                const long long rel = rel0 + (long long)k;
                if ((m >> k & 1u) && rel >= 0 && rel < (long long)need) s_id[rel] = (unsigned)v[k];
            }
        }

        // ---- position in the document and segment id, from the index alone
        if (docs) {
            const unsigned long long row0 = (unsigned long long)(p.pos ? p.pos[r] : s);
            const unsigned long long g0 = row0 + t0;
            for (unsigned e = tid; e < kBatchTile; e += kBatchThreads) s_flag[e] = 0;
            if (tid == 0) s_k[0] = lower_bound_u64(p.sep, p.n_sep, g0);
            if (tid == 64) s_k[1] = lower_bound_u64(p.sep, p.n_sep, g0 + len);
            if (tid == 128) s_k[2] = lower_bound_u64(p.sep, p.n_sep, row0);
            __syncthreads();
            const size_t k0 = s_k[0], k1 = s_k[1], kb = s_k[2];
            for (size_t j = k0 + tid; j < k1; j += kBatchThreads) {
                const unsigned long long d = p.sep[j] - g0;
                if (d < len) s_flag[d] = 1;   // (always, for a sorted index)
            }
            __syncthreads();
            int mx = -1;
            unsigned c = 0;
#pragma unroll
            for (unsigned q = 0; q < kPerThread; ++q) {
                const unsigned e = tid * kPerThread + q;
                if (e < len && s_flag[e]) {
                    mx = (int)e;
                    ++c;
                }
            }
            block_excl_max_sum(mx, c, s_wmx, s_wc);
            const long long last = k0 ? (long long)p.sep[k0 - 1] : -1ll;
            c += (unsigned)(k0 - kb);
#pragma unroll
            for (unsigned q = 0; q < kPerThread; ++q) {
                const unsigned e = tid * kPerThread + q;
                if (e < len) {
                    s_posn[e] = mx >= 0 ? (long long)e - mx - 1 : (long long)(g0 + e) - last - 1;
                    s_doc[e] = (int)c;
                    if (s_flag[e]) {
                        mx = (int)e;
                        ++c;
                    }
                }
            }
        }
        __syncthreads();

        // ---- both matrices from the one copy
        const size_t o0 = r * (size_t)p.row_len + t0;
        unsigned long long* st = p.status;
        store_tile(static_cast<O*>(p.inputs) + o0, len, [&](unsigned e) { return id_out<O>(s_id[e], st); });
        if (p.targets) {
            if (p.ignore) {
                const unsigned sep_id = p.sep_id;
                const O ign = (O)p.ignore_index;
                store_tile(static_cast<O*>(p.targets) + o0, len, [&](unsigned e) {
                    return s_id[e] == sep_id ? ign : id_out<O>(s_id[e + 1], st);
                });
            } else {
                store_tile(static_cast<O*>(p.targets) + o0, len,
                           [&](unsigned e) { return id_out<O>(s_id[e + 1], st); });
            }
        }
        if (p.positions) store_tile(p.positions + o0, len, [&](unsigned e) { return s_posn[e]; });
        if (p.doc_ids) store_tile(p.doc_ids + o0, len, [&](unsigned e) { return s_doc[e]; });
    }
}

template <class F>
int guarded_batch(F&& f) {
    try {
        f();
        set_error(0, "");
        return BPE_OK;
    } catch (const Error& e) {
        set_error(e.code, e.msg, e.sys_errno);
        return e.code;
    } catch (const std::bad_alloc&) {
        set_error(BPE_E_NOMEM, "host allocation failed");
        return BPE_E_NOMEM;
    } catch (const std::exception& e) {   // a copier thread that could not be started
        set_error(BPE_E_NOMEM, e.what());
        return BPE_E_NOMEM;
    }
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }

std::string bad_row_message(unsigned long long row, long long limit) {
    return "row " + std::to_string(row) + " starts outside [0, " + std::to_string(limit) + "]";
}

// Validates, enqueues the kernel on s and, with BPE_BATCH_CHECK, reads the status word back.
void batch_rows(const void* d_ids, size_t n, int elem_bytes, const int64_t* d_src, const int64_t* d_pos,
                const bpe_batch_args* a, hipStream_t s) {
    BPE_REQUIRE(a, BPE_E_ARG, "NULL argument");
    BPE_REQUIRE(elem_bytes == 2 || elem_bytes == 4, BPE_E_ARG, "ids must be 2 or 4 bytes each");
    BPE_REQUIRE(a->out_elem_bytes == 4 || a->out_elem_bytes == 8, BPE_E_ARG, "out_elem_bytes must be 4 or 8");
    BPE_REQUIRE((a->flags & ~(BPE_BATCH_CHECK | BPE_BATCH_IGNORE)) == 0, BPE_E_ARG, "unknown flags");
    BPE_REQUIRE(a->row_len >= 1 && a->row_len <= (size_t)INT32_MAX, BPE_E_ARG, "row_len must be in [1, 2^31)");
    BPE_REQUIRE(n < (1ull << 60), BPE_E_LIMIT, "too many ids");
    BPE_REQUIRE(aligned_to(d_ids, (size_t)elem_bytes), BPE_E_ARG, "ids are not aligned to their own size");
    const bool docs = a->d_positions || a->d_doc_ids;
    BPE_REQUIRE(!docs || a->n_sep == 0 || a->d_sep_pos, BPE_E_ARG, "NULL separator positions");
    const bool ignore = (a->flags & BPE_BATCH_IGNORE) != 0;
    BPE_REQUIRE(!ignore || a->d_targets, BPE_E_ARG, "ignore_index without targets");
    BPE_REQUIRE(!ignore || a->out_elem_bytes == 8 || (a->ignore_index >= INT32_MIN && a->ignore_index <= INT32_MAX),
                BPE_E_ARG, "ignore_index does not fit int32");
    const bool check = (a->flags & BPE_BATCH_CHECK) != 0;
    BPE_REQUIRE(!check || a->d_status, BPE_E_ARG, "BPE_BATCH_CHECK needs a status word");
    if (a->n_rows == 0) return;
    BPE_REQUIRE(a->n_rows <= SIZE_MAX / 8 / a->row_len, BPE_E_ARG, "n_rows x row_len overflows");
    BPE_REQUIRE(d_ids && d_src && a->d_inputs, BPE_E_ARG, "NULL argument");
    BPE_REQUIRE(aligned_to(a->d_inputs, (size_t)a->out_elem_bytes) && aligned_to(a->d_targets, (size_t)a->out_elem_bytes) &&
                    aligned_to(a->d_positions, 8) && aligned_to(a->d_doc_ids, 4) && aligned_to(a->d_status, 8) &&
                    aligned_to(d_src, 8) && aligned_to(d_pos, 8) && aligned_to(a->d_sep_pos, 8),
                BPE_E_ARG, "an array is not aligned to its element size");

    BatchParams p{};
    p.ids = d_ids;
    p.n = n;
    p.sh = (unsigned)((reinterpret_cast<uintptr_t>(d_ids) & 15u) / (size_t)elem_bytes);
    p.src = reinterpret_cast<const long long*>(d_src);
    p.pos = reinterpret_cast<const long long*>(d_pos);
    p.n_rows = a->n_rows;
    p.row_len = (unsigned)a->row_len;
    p.inputs = a->d_inputs;
    p.targets = a->d_targets;
    p.positions = reinterpret_cast<long long*>(a->d_positions);
    p.doc_ids = a->d_doc_ids;
    p.sep = reinterpret_cast<const unsigned long long*>(a->d_sep_pos);
    p.n_sep = a->n_sep;
    // a separator id that no element can hold matches nothing
    const bool sep_fits = elem_bytes == 2 ? a->separator_id <= 0xFFFFu : a->separator_id <= 0xFFFFFFFFull;
    p.sep_id = (unsigned)a->separator_id;
    p.ignore = ignore && sep_fits;
    p.ignore_index = a->ignore_index;
    p.status = reinterpret_cast<unsigned long long*>(a->d_status);

    if (p.status) BPE_HIP(hipMemsetAsync(p.status, 0xFF, 8, s));
    const size_t tiles = a->n_rows * ((a->row_len + kBatchTile - 1) / kBatchTile);
    const unsigned grid = (unsigned)std::min<size_t>(tiles, kMaxGridBlocks);
    if (elem_bytes == 2) {
        if (a->out_elem_bytes == 4) hipLaunchKernelGGL((k_batch_rows<uint16_t, int32_t>), dim3(grid), dim3(kBatchThreads), 0, s, p);
        else hipLaunchKernelGGL((k_batch_rows<uint16_t, long long>), dim3(grid), dim3(kBatchThreads), 0, s, p);
    } else {
        if (a->out_elem_bytes == 4) hipLaunchKernelGGL((k_batch_rows<uint32_t, int32_t>), dim3(grid), dim3(kBatchThreads), 0, s, p);
        else hipLaunchKernelGGL((k_batch_rows<uint32_t, long long>), dim3(grid), dim3(kBatchThreads), 0, s, p);
    }
    BPE_HIP(hipGetLastError());
    if (!check) return;
    unsigned long long got = ~0ull;
    BPE_HIP(hipMemcpyAsync(&got, p.status, 8, hipMemcpyDeviceToHost, s));
    BPE_HIP(hipStreamSynchronize(s));
    if (got == ~0ull) return;
    const long long limit = (long long)n - (long long)a->row_len - (a->d_targets ? 1 : 0);
    BPE_REQUIRE(got >= kLimitBit, BPE_E_ARG, bad_row_message(got, limit));
    throw Error{BPE_E_LIMIT, "token id " + std::to_string(got & 0xFFFFFFFFull) +
                                 " does not fit int32 rows (ids from 2^31 on need out_elem_bytes 8)"};
}

constexpr unsigned kStageThreads = 8;            // at most; never sized by the machine's CPU count
constexpr size_t kStageBytesPerThread = 512u << 10;

struct StageSlot {
    uint8_t* pinned = nullptr;
    size_t pinned_bytes = 0;
    DevBuf<uint8_t> dev;
    hipEvent_t done = nullptr;
    bool in_flight = false;
};

}  // namespace
}  // namespace bpe

struct bpe_batch_stage {
    int device = 0;
    bpe::StageSlot slot[2];
    unsigned next = 0;
    ~bpe_batch_stage() {
        for (auto& sl : slot) {
            if (sl.in_flight) (void)hipEventSynchronize(sl.done);
            if (sl.done) (void)hipEventDestroy(sl.done);
            if (sl.pinned) (void)hipHostFree(sl.pinned);
        }
    }
};

extern "C" {

int bpe_ids_batch_rows_device(const void* d_ids, size_t n, int elem_bytes, const int64_t* d_src, const int64_t* d_pos,
                              const bpe_batch_args* args, void* hip_stream) {
    return bpe::guarded_batch([&] { bpe::batch_rows(d_ids, n, elem_bytes, d_src, d_pos, args, (hipStream_t)hip_stream); });
}

int bpe_batch_stage_create(bpe_batch_stage** out) {
    return bpe::guarded_batch([&] {
        BPE_REQUIRE(out, BPE_E_ARG, "NULL argument");
        *out = nullptr;
        std::unique_ptr<bpe_batch_stage> st(new bpe_batch_stage());
        BPE_HIP(hipGetDevice(&st->device));
        for (auto& sl : st->slot) BPE_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        *out = st.release();
    });
}

int bpe_batch_stage_rows(bpe_batch_stage* st, const void* ids, size_t n, int elem_bytes, const int64_t* starts,
                         const bpe_batch_args* args, void* hip_stream) {
    return bpe::guarded_batch([&] {
        BPE_REQUIRE(st && args, BPE_E_ARG, "NULL argument");
        BPE_REQUIRE(elem_bytes == 2 || elem_bytes == 4, BPE_E_ARG, "ids must be 2 or 4 bytes each");
        BPE_REQUIRE(args->row_len >= 1 && args->row_len <= (size_t)INT32_MAX, BPE_E_ARG, "row_len must be in [1, 2^31)");
        int dev = 0;
        BPE_HIP(hipGetDevice(&dev));
        BPE_REQUIRE(dev == st->device, BPE_E_ARG, "the staging handle belongs to another device");
        hipStream_t s = (hipStream_t)hip_stream;
        const size_t B = args->n_rows;
        if (B == 0) {
            bpe::batch_rows(nullptr, 0, elem_bytes, nullptr, nullptr, args, s);   // the argument checks
            return;
        }
        BPE_REQUIRE(ids && starts, BPE_E_ARG, "NULL argument");
        const size_t span = args->row_len + (args->d_targets ? 1 : 0);
        BPE_REQUIRE(B <= (SIZE_MAX / 16) / span, BPE_E_ARG, "n_rows x row_len overflows");
        const long long limit = (long long)n - (long long)span;
        for (size_t r = 0; r < B; ++r)
            BPE_REQUIRE(starts[r] >= 0 && starts[r] <= limit, BPE_E_ARG, bpe::bad_row_message(r, limit));

        bpe::StageSlot& sl = st->slot[st->next];
        st->next ^= 1u;
        if (sl.in_flight) {   // the copy and the kernel that last used this pair of buffers
            BPE_HIP(hipEventSynchronize(sl.done));
            sl.in_flight = false;
        }
        // [src: B x int64][pos: B x int64][ids: B spans], moved by one copy
        const size_t head = 16 * B, row_bytes = span * (size_t)elem_bytes, total = head + B * row_bytes;
        if (total > sl.pinned_bytes) {
            if (sl.pinned) (void)hipHostFree(sl.pinned);
            sl.pinned = nullptr;
            sl.pinned_bytes = 0;
            const size_t want = std::max(total + total / 2, (size_t)64 << 10);
            BPE_HIP(hipHostMalloc(reinterpret_cast<void**>(&sl.pinned), want, hipHostMallocDefault));
            sl.pinned_bytes = want;
        }
        if (total > sl.dev.n) sl.dev.alloc(std::max(total + total / 2, (size_t)64 << 10));
        int64_t* h_src = reinterpret_cast<int64_t*>(sl.pinned);
        int64_t* h_pos = h_src + B;
        for (size_t r = 0; r < B; ++r) {
            h_src[r] = (int64_t)(r * span);
            h_pos[r] = starts[r];
        }
        const uint8_t* base = static_cast<const uint8_t*>(ids);
        uint8_t* dst = sl.pinned + head;
        auto copy_rows = [&](size_t lo, size_t hi) {
            for (size_t r = lo; r < hi; ++r)
                std::memcpy(dst + r * row_bytes, base + (size_t)starts[r] * (size_t)elem_bytes, row_bytes);
        };
        const size_t want_thr = std::min<size_t>(std::min<size_t>(bpe::kStageThreads, B),
                                                 std::max<size_t>(1, B * row_bytes / bpe::kStageBytesPerThread));
        if (want_thr <= 1) {
            copy_rows(0, B);
        } else {
            std::vector<std::thread> pool;
            pool.reserve(want_thr - 1);
            const size_t per = (B + want_thr - 1) / want_thr;
            for (size_t t = 1; t < want_thr; ++t)
                pool.emplace_back(copy_rows, std::min(B, t * per), std::min(B, (t + 1) * per));
            copy_rows(0, std::min(B, per));
            for (auto& th : pool) th.join();
        }
        BPE_HIP(hipMemcpyAsync(sl.dev.p, sl.pinned, total, hipMemcpyHostToDevice, s));
        sl.in_flight = true;   // (also when the launch below fails: the copy reads the pinned buffer)
        struct Mark {
            bpe::StageSlot& sl;
            hipStream_t s;
            ~Mark() { (void)hipEventRecord(sl.done, s); }
        } mark{sl, s};
        bpe::batch_rows(sl.dev.p + head, B * span, elem_bytes, reinterpret_cast<const int64_t*>(sl.dev.p),
                        reinterpret_cast<const int64_t*>(sl.dev.p) + B, args, s);
    });
}

void bpe_batch_stage_free(bpe_batch_stage* st) { delete st; }

}  // extern "C"
