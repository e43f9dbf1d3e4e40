// Masked language modelling: the tied projection + cross-entropy on the LABELLED rows only.
//
// The reference's MaskedLMModel (virtex/models/masked_lm.py:33,67-72) projects all B*T decoder rows onto the vocabulary and
// hands them to nn.CrossEntropyLoss(ignore_index = padding_idx); its dataset labels ceil((len - 2) * 0.15) <= 5 of 30 positions
// per caption (virtex/data/datasets/masked_lm.py:73-76), so about five rows in six carry padding_idx, contribute nothing to the
// loss and get an exactly-zero gradient.  The three kernels here move the labelled rows into a dense [cap][H] operand and back;
// between them the EXISTING entry points run unchanged on cap rows instead of B*T: vtx_tied_ce_fwd / _bwd, vtx_gemm_nt for
// d(packed), vtx_gemm_tn_acc for the tied word matrix.  "Labelled" is the rule of ce_lse_combine_kernel (tied_ce.hip):
// label != ignore_index && 0 <= label < V.
//
// label_compact: a STABLE compaction in one launch and without atomics, so rows[] is ascending and the result is
// bit-reproducible.  One block of 1 024 threads (16 waves) walks the label vector in strips of 1 024 rows.  Per strip: every lane
// evaluates the rule for its row, a wave ballot gives the wave's 64-bit mask, the popcount of the bits below the lane is the
// lane's rank inside the wave, the 16 wave totals meet in LDS (64 bytes) where every thread adds up the waves in front of its
// own, and a running carry (the same register value in every thread) passes from strip to strip.  R = B*T reaches 30 720 at the
// largest supported batch: 30 strips, two barriers each -- a second block could not start before the first one's total is known.
//
// rows_pack / rows_unpack: pure 16-byte copies, dtype-blind (a row is H * sizeof(T) / 16 vectors).  A thread owns four vectors
// 256 apart in the flattened [row][vector] space; it requests its four row indices, then its four data vectors (addresses of
// rows that do not exist clamped to row 0, values masked afterwards), and only then stores: two dependent memory latencies per
// thread instead of eight.  count is read from device memory -- the host never needs it for the launch.
//   pack  : packed[i] = hidden[rows[i]], packed_targets[i] = labels[rows[i]] for i < min(count, cap); the other rows of the cap
//           are zeros with target ignore_index, which the loss kernels skip like any ignored row.  count > cap (a static capacity
//           that the batch exceeds): packed row 0 -- a labelled row then -- is filled with NaN, so its target logit, its row loss
//           and the mean are NaN: never a silently truncated mean, and no host synchronisation to find out.
//   unpack: dfull[r] = slot[r] in [0, cap) ? dpacked[slot[r]] : 0 -- every row of dfull written exactly once (no memset, no
//           atomics).
#include "vtx_common.h"

namespace {

constexpr int LC_THREADS = 1024, LC_WAVES = LC_THREADS / 64;
constexpr int LC_MAX_R = 1 << 20;      // accepted range of R (1 024 strips; the supported batches need 30)
constexpr int RP_THREADS = 256, RP_UNROLL = 4;

__device__ __forceinline__ bool is_labelled(long long v, int ignore_index, int V) { return v != ignore_index && v >= 0 && v < V; }

__global__ __launch_bounds__(LC_THREADS) void label_compact_kernel(const long long* __restrict__ labels, int ignore_index, int V,
                                                                    int* __restrict__ rows, int* __restrict__ slot,
                                                                    int* __restrict__ count, int R) {
    __shared__ int wave_total[LC_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int carry = 0;                                             // labelled rows in the strips behind this one
    for (int r0 = 0; r0 < R; r0 += LC_THREADS) {
        const int r = r0 + t;
        const bool lab = r < R && is_labelled(labels[r < R ? r : 0], ignore_index, V);
        const unsigned long long mask = __ballot(lab);
        const int rank = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[w] = __builtin_popcountll(mask);
        __syncthreads();
        int before = carry, strip = 0;
#pragma unroll
        for (int k = 0; k < LC_WAVES; ++k) {
            const int x = wave_total[k];                       // LDS broadcast
            before += k < w ? x : 0;
            strip += x;
        }
        if (r < R) {
            slot[r] = lab ? before + rank : -1;
            if (lab) rows[before + rank] = r;
        }
        carry += strip;
        __syncthreads();                                       // the totals have been read: the next strip may overwrite them
    }
    if (t == 0) count[0] = carry;
}

// nv: 16-byte vectors per row; ldv: row stride of `hidden` in vectors
__global__ __launch_bounds__(RP_THREADS) void rows_pack_kernel(const uint4* __restrict__ hidden, long ldv,
                                                               const long long* __restrict__ labels, const int* __restrict__ rows,
                                                               const int* __restrict__ count, int cap, uint4* __restrict__ packed,
                                                               long long* __restrict__ packed_targets, int ignore_index, int nv,
                                                               uint32_t nan_word) {
    const int cnt = count[0];
    const int n = cnt < cap ? cnt : cap;
    const bool overflow = cnt > cap;
    const int total = cap * nv;
    const int base = blockIdx.x * (RP_THREADS * RP_UNROLL) + threadIdx.x;
    int row[RP_UNROLL], vec[RP_UNROLL], src[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        const int idx = base + u * RP_THREADS;
        row[u] = (idx < total ? idx : 0) / nv;
        vec[u] = (idx < total ? idx : 0) - row[u] * nv;
        src[u] = rows[row[u] < n ? row[u] : 0];                // rows[0] may be unwritten (count == 0): masked below, never an address
    }
    vtx_loads_issued();
    uint4 raw[RP_UNROLL];
    long long tgt[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        const int s = row[u] < n ? src[u] : 0;                 // a filler row reads row 0 of hidden, which always exists
        raw[u] = hidden[(long)s * ldv + vec[u]];
        tgt[u] = labels[s];
    }
    vtx_loads_issued();
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        if (base + u * RP_THREADS < total) {
            const bool live = row[u] < n;
            uint4 o = live ? raw[u] : make_uint4(0u, 0u, 0u, 0u);
            if (overflow && row[u] == 0) o = make_uint4(nan_word, nan_word, nan_word, nan_word);
            packed[(long)row[u] * nv + vec[u]] = o;
            if (vec[u] == 0) packed_targets[row[u]] = live ? tgt[u] : (long long)ignore_index;
        }
    }
}

__global__ __launch_bounds__(RP_THREADS) void rows_unpack_kernel(const uint4* __restrict__ dpacked, const int* __restrict__ slot,
                                                                 int cap, uint4* __restrict__ dfull, long lddv, int R, int nv) {
    const int total = R * nv;
    const int base = blockIdx.x * (RP_THREADS * RP_UNROLL) + threadIdx.x;
    int row[RP_UNROLL], vec[RP_UNROLL], s[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        const int idx = base + u * RP_THREADS;
        row[u] = (idx < total ? idx : 0) / nv;
        vec[u] = (idx < total ? idx : 0) - row[u] * nv;
        s[u] = slot[row[u]];
    }
    vtx_loads_issued();
    uint4 raw[RP_UNROLL];
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        const bool live = s[u] >= 0 && s[u] < cap;             // a slot beyond a static capacity has no packed row
        raw[u] = dpacked[(long)(live ? s[u] : 0) * nv + vec[u]];
    }
    vtx_loads_issued();
#pragma unroll
    for (int u = 0; u < RP_UNROLL; ++u) {
        if (base + u * RP_THREADS < total) {
            const bool live = s[u] >= 0 && s[u] < cap;
            dfull[(long)row[u] * lddv + vec[u]] = live ? raw[u] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows x vectors of one launch must index in 31 bits
int copy_shape(const char* who, int dtype, long nrows, int H, long ld, int* nv, long* ldv) {
    VTX_CHECK(dtype == VTX_BF16 || dtype == VTX_F32, VTX_ERR_DTYPE, "%s: bad dtype %d", who, dtype);
    const int vec = dtype == VTX_BF16 ? 8 : 4;
    VTX_CHECK(H > 0 && H % vec == 0 && ld >= H && ld % vec == 0, VTX_ERR_SHAPE, "%s: H = %d and the row stride %ld must be multiples of %d", who,
              H, ld, vec);
    *nv = H / vec;
    *ldv = ld / vec;
    VTX_CHECK(nrows * *nv < (1L << 31) - RP_THREADS * RP_UNROLL, VTX_ERR_SHAPE, "%s: %ld rows x %d vectors exceed 2^31", who, nrows, *nv);
    return VTX_OK;
}

}  // namespace

extern "C" int vtx_label_compact(const long long* labels, int ignore_index, int V, int* rows, int* slot, int* count, int R,
                                 void* stream) {
    VTX_CHECK(labels && rows && slot && count, VTX_ERR_ARG, "label_compact: null pointer");
    VTX_CHECK(V > 0, VTX_ERR_ARG, "label_compact: bad V = %d", V);
    VTX_CHECK(R >= 1 && R <= LC_MAX_R, VTX_ERR_SHAPE, "label_compact: R = %d outside [1, %d] (one block walks the labels)", R, LC_MAX_R);
    VTX_KLAUNCH("label_compact", 0, 16.0 * R, label_compact_kernel, dim3(1), dim3(LC_THREADS), 0, (hipStream_t)stream, labels, ignore_index, V,
                rows, slot, count, R);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

extern "C" int vtx_rows_pack(int dtype, const void* hidden, long ldh, const long long* labels, const int* rows, const int* count,
                             int cap, void* packed, long long* packed_targets, int ignore_index, int H, void* stream) {
    VTX_CHECK(hidden && labels && rows && count && packed && packed_targets, VTX_ERR_ARG, "rows_pack: null pointer");
    VTX_CHECK(cap >= 1, VTX_ERR_ARG, "rows_pack: capacity %d < 1", cap);
    int nv;
    long ldv;
    if (int rc = copy_shape("rows_pack", dtype, cap, H, ldh, &nv, &ldv)) return rc;
    VTX_CHECK(aligned16(hidden) && aligned16(packed), VTX_ERR_SHAPE, "rows_pack: operands must be 16-byte aligned");
    const uint32_t nan_word = dtype == VTX_BF16 ? 0x7fc07fc0u : 0x7fc00000u;
    VTX_KLAUNCH("rows_pack", 0, 32.0 * cap * nv, rows_pack_kernel, dim3(vtx_cdiv((long)cap * nv, RP_THREADS * RP_UNROLL)), dim3(RP_THREADS), 0,
                (hipStream_t)stream, (const uint4*)hidden, ldv, labels, rows, count, cap, (uint4*)packed, packed_targets, ignore_index, nv,
                nan_word);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}

extern "C" int vtx_rows_unpack(int dtype, const void* dpacked, const int* slot, int cap, void* dfull, long ldd, int R, int H,
                               void* stream) {
    VTX_CHECK(dpacked && slot && dfull, VTX_ERR_ARG, "rows_unpack: null pointer");
    VTX_CHECK(cap >= 1 && R >= 1, VTX_ERR_ARG, "rows_unpack: bad shape cap = %d, R = %d", cap, R);
    int nv;
    long lddv;
    if (int rc = copy_shape("rows_unpack", dtype, R, H, ldd, &nv, &lddv)) return rc;
    VTX_CHECK(aligned16(dpacked) && aligned16(dfull), VTX_ERR_SHAPE, "rows_unpack: operands must be 16-byte aligned");
    VTX_KLAUNCH("rows_unpack", 0, 16.0 * R * nv + 16.0 * cap * nv, rows_unpack_kernel, dim3(vtx_cdiv((long)R * nv, RP_THREADS * RP_UNROLL)),
                dim3(RP_THREADS), 0, (hipStream_t)stream, (const uint4*)dpacked, slot, cap, (uint4*)dfull, lddv, R, nv);
    VTX_LAUNCH_CHECK();
    return VTX_OK;
}
